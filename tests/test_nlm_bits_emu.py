"""The bits of the NL-means filter body in the host emulation, held to the word: dn_filter_block (denoise_kernels.h) as k_dn_filter,
k_dn_filter_halves, k_tdn_pass and k_gdn_filter run it, on films that depend on nothing but integer arithmetic.

tests/golden/nlm_bits.txt holds one line per call, its name and the sha256 of the output's words (little-endian uint32). It was recorded from
the headers as they were BEFORE the four kernels came to share one body (each of the temporal and the guided kernel then had a copy of it), and
it is never recorded again from the code under test: a change of the body that moves one bit of one call fails here, and has to be justified as
a change of the filter, with a new file recorded from the code before it.

Films: a 32-bit LCG over np.uint32 (Numerical Recipes' constants); a colour channel is (state >> 8) * 2^-24, the weight is 1 + (state >> 29), the
film holds (colour * weight, weight); no libm, no numpy random stream. Pixels of weight 0, of negative weight and with a NaN colour sit at fixed
positions. Shapes: 67 x 45 (3 x 3 blocks, partial on the right and at the bottom) and 9 x 5 (less than one 32 x 16 tile and less than the larger
radii: the whole halo lies outside the image)."""
import hashlib
import os

import numpy as np
import pytest

import _emu_features as EF
import _guided_ref as G
import _temporal_ref as TR

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlm_bits.txt")
SHAPES = [(67, 45), (9, 5)]
RTF = [(1, 1, 0), (3, 2, 1), (7, 3, 3), (10, 7, 3)]   # (radius, temporal radius, patch)
K, SECOND = 0.45, (5, 1, 1.0)   # k of the plain, halves and temporal calls and of the first pass; the guided call has k = 1.0, the second pass SECOND


def lcg(seed, n):
    """n successive states of x <- 1664525 x + 1013904223 (mod 2^32) after `seed`"""
    out = np.empty(n, np.uint32)
    s = int(seed) & 0xFFFFFFFF
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = s
    return out


def film(w, h, seed):
    s = lcg(seed, w * h * 4).reshape(h, w, 4)
    col = (s[..., :3] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    wgt = (F32(1) + (s[..., 3] >> np.uint32(29)).astype(F32))[..., None]
    return np.ascontiguousarray(np.concatenate([col * wgt, wgt], -1).astype(F32))


def films(w, h, seed):
    """an (even, odd) pair; the invalid pixels lie inside 9 x 5, and at a tile's corner, in a partial tile and in the last pixel where there is room"""
    even, odd = film(w, h, 2 * seed + 1), film(w, h, 2 * seed + 2)
    shift = seed % 3   # (another seed, other invalid pixels)
    even[1, 2 + shift] = 0.0                 # no sample landed
    odd[4, shift, 3] = 0.0
    odd[3, 5 + shift] *= F32(-1.0)           # negative weight
    even[2, 6 + shift, 1] = np.nan           # a NaN colour
    if w > 40 and h > 20:
        even[16, 32 + shift, 3] = 0.0
        odd[20, 40 + shift] *= F32(-1.0)
        even[h - 1, w - 1, 0] = np.nan
        odd[15, 31 - shift, 2] = np.nan
    return even, odd


def digest(*outs):
    m = hashlib.sha256()
    for x in outs:
        m.update(np.ascontiguousarray(x, F32).view(np.uint32).astype("<u4").tobytes())
    return m.hexdigest()


def calls(w, h, r, rt, f):
    """(name, digest) of the five calls at one shape and setting"""
    tag = f"{w}x{h} r{r} t{rt} f{f}"
    frames = [films(w, h, seed) for seed in (1, 2, 3)]
    even, odd = frames[0]
    ga, gb = films(w, h, 7)
    guided = G.guided_lib()
    yield f"denoise {tag}", digest(EF.denoise(EF.denoise_lib(), even, odd, r, f, K))
    yield f"halves {tag}", digest(*EF.guide_halves(EF.guide_lib(), even, odd, r, f, K))
    yield f"temporal {tag}", digest(TR.run(TR.temporal_lib(), frames, r, rt, f, K))
    yield f"guided {tag}", digest(G.run_guided(guided, even, odd, ga, gb, r, f, 1.0))
    yield f"two_pass {tag}", digest(G.run_two_pass(guided, even, odd, r, f, K, *SECOND))


def golden():
    with open(GOLDEN) as fh:
        lines = [l.rstrip("\n") for l in fh if l.strip() and not l.startswith("#")]
    return dict(l.rsplit(" ", 1) for l in lines)


def test_the_generator_is_integer_arithmetic():
    """the first states of the LCG and what a film makes of them, stated here as numbers"""
    assert lcg(0, 4).tolist() == [0x3C6EF35F, 0x47502932, 0xD1CCF6E9, 0xAAF95334]
    # the first pixel: weight 1 + (0xAAF95334 >> 29) = 6, colours (state >> 8) / 2^24 times it, each rounded to float32 once
    assert film(2, 1, 0)[0, 0].tolist() == [float(F32(c * 2.0 ** -24) * F32(6)) for c in (3960563, 4673577, 13749494)] + [6.0]


@pytest.mark.parametrize("r,rt,f", RTF, ids=[f"r{r}t{rt}f{f}" for r, rt, f in RTF])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_the_filters_bits_are_the_recorded_ones(w, h, r, rt, f):
    want = golden()
    assert len(want) == 5 * len(SHAPES) * len(RTF)
    for name, got in calls(w, h, r, rt, f):
        assert got == want[name], name
