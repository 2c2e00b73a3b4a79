"""bench.py --dump-outputs: what it writes (float32 films, or a seeded pixel sample of them) stays under 64 MB in all and is the
same from run to run, so that two builds can be compared output for output."""
import os

import numpy as np

import bench

CAP = 64 * 10**6


def _films(n):
    rng = np.random.default_rng(3)
    return [(f"film_frame{i}", rng.random((bench.HEIGHT, bench.WIDTH, 4), dtype=np.float32)) for i in range(n)]


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_one_film_is_written_whole(tmp_path):
    films = _films(1)
    names = bench.dump_outputs(str(tmp_path), films)
    assert names == ["film_frame0"]
    got = np.load(tmp_path / "film_frame0.npy")
    assert got.dtype == np.float32 and (got == films[0][1]).all()
    assert _sizes(str(tmp_path)) <= CAP


def test_a_larger_output_is_sampled_the_same_way_every_run(tmp_path):
    films = _films(3)
    a, b = tmp_path / "a", tmp_path / "b"
    names = bench.dump_outputs(str(a), films)
    assert names == bench.dump_outputs(str(b), films)
    assert names == ["sample_pixel_index"] + [f"film_frame{i}_sample" for i in range(3)]
    assert _sizes(str(a)) <= CAP
    idx = np.load(a / "sample_pixel_index.npy")
    assert idx.dtype == np.float64 and (idx == np.load(b / "sample_pixel_index.npy")).all()
    pix = idx.astype(np.int64)
    assert (np.diff(pix) > 0).all() and pix[-1] < bench.WIDTH * bench.HEIGHT
    for i, (name, f) in enumerate(films):
        got = np.load(a / f"{name}_sample.npy")
        assert got.dtype == np.float32 and got.shape == (len(pix), 4)
        assert (got == f.reshape(-1, 4)[pix]).all() and (got == np.load(b / f"{name}_sample.npy")).all()


def test_ranks_of_a_frame_sequence_share_one_dump(tmp_path):
    """--gpus 2 --workload tr15_like --frames 5: the ranks hold 3 and 2 frames (multi.shard_frames). Each reduces its own frames
    with the index of the WHOLE sequence, rank 0 writes them all: one index that fits every sample, one budget for all."""
    from tray_rust_amd import multi
    first, n, world = 63, 5, 2
    rng = np.random.default_rng(4)
    films = {fr: rng.random((bench.HEIGHT, bench.WIDTH, 4), dtype=np.float32) for fr in range(first, first + n)}
    shares = []
    for rank in range(world):
        idx = bench.dump_index(n)   # what each rank computes for itself
        shares.append([(f"film_frame{fr}", bench.reduce_film(films[fr], idx)) for fr in multi.shard_frames(first, first + n - 1, rank, world)])
    assert sorted(len(s) for s in shares) == [2, 3]
    gathered = bench.merge_shares(shares[::-1])   # (in whatever order the shares arrive)
    names = bench.write_dump(str(tmp_path), gathered, bench.dump_index(n))
    assert names == ["sample_pixel_index"] + [f"film_frame{fr}_sample" for fr in range(first, first + n)]
    assert _sizes(str(tmp_path)) <= CAP
    pix = np.load(tmp_path / "sample_pixel_index.npy").astype(np.int64)
    for fr, f in films.items():
        assert (np.load(tmp_path / f"film_frame{fr}_sample.npy") == f.reshape(-1, 4)[pix]).all()


def test_two_whole_films_do_not_exceed_the_budget(tmp_path):
    """--gpus 2 --frames 2: one frame per rank, 2 x 33 MB whole would pass 64 MB -- the pair is sampled"""
    films = _films(2)
    idx = bench.dump_index(2)
    assert idx is not None
    bench.write_dump(str(tmp_path), [(name, bench.reduce_film(f, idx)) for name, f in films], idx)
    assert _sizes(str(tmp_path)) <= CAP
