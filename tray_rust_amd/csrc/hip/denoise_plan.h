// What the thirteen tray_denoise_*_device calls (include/trayhip.h) decide on the host: which arguments they refuse, where the regions of their scratch
// buffers lie, and which launches they make in which order. Host-only functions of the calls' plain arguments -- no HIP call, no stream, no kernel
// header: device_api.hip runs the schedules with an Ops that forwards to the add-on libraries' launch functions (denoise.h, guide.h, guided.h,
// temporal.h, tdemod.h, t2pass.h, td2pass.h, first_hit.h), the host emulation (tests/emu) compiles this header under g++ and runs the same schedules
// with an Ops that launches the kernels as fibers (tests/emu/emu_denoise_ops.h). A call's rules, layout and schedule are written here once; an add-on
// library brings its kernels and their launch functions. The schedules are templates: an Ops needs only the members that the schedules run with it call.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../../include/trayhip.h"

namespace tr_dnplan {

// ---- the calls' arguments

struct Params { uint32_t radius, radius_t, patch; float k; };   // one pass's; radius_t: a temporal call's window in the neighbouring frames
struct Frame { const float* even, * odd, * albedo, * guide_a, * guide_b; };   // the films one frame brings (null: the call has no such film)
struct Neighbours {   // the host arrays of the neighbouring frames' films, n pointers each (null: the call has no such array)
    uint32_t n;
    const float* const* even, * const* odd, * const* albedo, * const* guide_a, * const* guide_b;
    Frame operator[](uint32_t j) const {
        return {even ? even[j] : nullptr, odd ? odd[j] : nullptr, albedo ? albedo[j] : nullptr, guide_a ? guide_a[j] : nullptr, guide_b ? guide_b[j] : nullptr};
    }
};
// what a call is: the films its frames bring besides (even, odd), and which rules hold for it
enum : uint32_t {
    kAlbedo = 1u,          // an albedo film per frame
    kGuide = 2u,           // a guide pair per frame
    kTemporal = 4u,        // neighbouring frames: radius_t and N have rules
    kGuideMayAlias = 8u,   // the inputs are only read: a frame's guide may be its own films (then a guided call is the unguided one)
};
constexpr uint32_t kMaxBuffers = 5u * (TRAY_DENOISE_MAX_NEIGHBOURS + 1u) + 3u;   // five films per frame, two outputs and the scratch buffer

// ---- rules: {TRAY_OK, ""} or the refusal's return code and message

struct Refusal { int rc; std::string msg; };

// the filter's own argument rules (tray_denoise_device's), shared by the calls that take them; `who` names the call in the message
inline Refusal filter_args(const std::string& who, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k) {
    if (width == 0u || height == 0u) return {TRAY_E_INVALID, who + ": width and height must be >= 1"};
    if (radius < 1u || radius > 10u || patch > 3u) return {TRAY_E_INVALID, who + ": 1 <= radius <= 10 and patch <= 3 are required"};
    if (!(k > 0.0f) || !std::isfinite(k)) return {TRAY_E_INVALID, who + ": k must be > 0 and finite"};
    return {TRAY_OK, ""};
}
// the temporal calls' rules for (radius, radius_t, patch, k) and for N
inline Refusal temporal_args(const std::string& who, uint32_t width, uint32_t height, uint32_t n_neighbours, uint32_t radius, uint32_t radius_t, uint32_t patch,
                             float k) {
    if (Refusal r = filter_args(who, width, height, radius, patch, k); r.rc != TRAY_OK) return r;
    if (radius_t < 1u || radius_t > radius) return {TRAY_E_INVALID, who + ": 1 <= radius_t <= radius is required"};
    if (n_neighbours > TRAY_DENOISE_MAX_NEIGHBOURS) return {TRAY_E_INVALID, who + ": at most " + std::to_string(TRAY_DENOISE_MAX_NEIGHBOURS) + " neighbouring frames"};
    return {TRAY_OK, ""};
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }
// n buffers, pairwise different and 16-byte aligned
inline bool distinct_aligned(const void* const* bufs, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!aligned16(bufs[i])) return false;
        for (size_t j = 0; j < i; ++j)
            if (bufs[i] == bufs[j]) return false;
    }
    return true;
}
// the looser rule of the calls with kGuideMayAlias over n_frames frames of `stride` films each (even, odd first, the guide pair last): the two
// films of a pair differ, the outputs and the scratch buffer differ from every film and from each other, and all are 16-byte aligned
inline bool guided_buffers(const void* const* outs, uint32_t n_outs, const void* const* films, uint32_t stride, uint32_t n_frames) {
    bool ok = distinct_aligned(outs, n_outs);
    for (uint32_t f = 0; f < n_frames; ++f) {
        const void* const* in = films + (size_t)stride * f;
        ok = ok && in[0] != in[1] && in[stride - 2u] != in[stride - 1u];
        for (uint32_t i = 0; i < stride; ++i) {
            ok = ok && aligned16(in[i]);
            for (uint32_t o = 0; o < n_outs; ++o) ok = ok && in[i] != outs[o];
        }
    }
    return ok;
}
// the films of a frame of a call, in the order (even, odd, albedo, guide_a, guide_b); returns their number
inline uint32_t films_of(const Frame& f, uint32_t what, const void** films) {
    uint32_t n = 0;
    films[n++] = f.even; films[n++] = f.odd;
    if (what & kAlbedo) films[n++] = f.albedo;
    if (what & kGuide) { films[n++] = f.guide_a; films[n++] = f.guide_b; }
    return n;
}

// The rules of every call but tray_denoise_device, in the order the calls have always checked them: no null film of the centre, output or scratch
// buffer (`outs`: the outputs, then the scratch buffer); the pass's parameters, then the second pass's; no null array and no null film of a
// neighbour; the buffers all different (or guided_buffers) and aligned -- `differ` is the call's own sentence about that.
inline Refusal call_rules(const std::string& who, uint32_t what, uint32_t width, uint32_t height, const Frame& centre, const Neighbours& nb, const Params& p,
                          const Params* second, std::initializer_list<const void*> outs, const char* differ) {
    const void* bufs[kMaxBuffers];
    uint32_t n = 0;
    for (const void* o : outs) bufs[n++] = o;
    const uint32_t n_outs = n, stride = films_of(centre, what, bufs + n);
    n += stride;
    for (uint32_t i = 0; i < n; ++i)
        if (!bufs[i]) return {TRAY_E_INVALID, who + ": null argument"};
    auto pass_args = [&](const std::string& w, const Params& q) {
        return (what & kTemporal) ? temporal_args(w, width, height, nb.n, q.radius, q.radius_t, q.patch, q.k) : filter_args(w, width, height, q.radius, q.patch, q.k);
    };
    if (Refusal r = pass_args(who, p); r.rc != TRAY_OK) return r;
    if (second)
        if (Refusal r = pass_args(who + ", second pass", *second); r.rc != TRAY_OK) return r;
    if (nb.n > 0u && (!nb.even || !nb.odd || ((what & kAlbedo) && !nb.albedo) || ((what & kGuide) && (!nb.guide_a || !nb.guide_b))))
        return {TRAY_E_INVALID, who + ": null argument"};
    for (uint32_t j = 0; j < nb.n; ++j, n += stride) {
        films_of(nb[j], what, bufs + n);
        for (uint32_t i = 0; i < stride; ++i)
            if (!bufs[n + i]) return {TRAY_E_INVALID, who + ": null film of a neighbouring frame"};
    }
    const bool ok = (what & kGuideMayAlias) ? guided_buffers(bufs, n_outs, bufs + n_outs, stride, nb.n + 1u) : distinct_aligned(bufs, n);
    if (!ok) return {TRAY_E_INVALID, who + ": " + differ};
    return {TRAY_OK, ""};
}

// tray_denoise_device's own: "different" and "aligned" are two messages, and the scratch buffer is not compared with the films
inline Refusal denoise_rules(uint32_t width, uint32_t height, const float* even, const float* odd, const Params& p, const float* out, const void* scratch) {
    if (!even || !odd || !out || !scratch) return {TRAY_E_INVALID, "tray_denoise_device: null argument"};
    if (Refusal r = filter_args("tray_denoise_device", width, height, p.radius, p.patch, p.k); r.rc != TRAY_OK) return r;
    if (even == odd || out == even || out == odd) return {TRAY_E_INVALID, "tray_denoise_device: the two films and the output must be three different buffers"};
    if (!aligned16(even) || !aligned16(odd) || !aligned16(out) || !aligned16(scratch))
        return {TRAY_E_INVALID, "tray_denoise_device: the films, the output and the scratch buffer must be 16-byte aligned"};
    return {TRAY_OK, ""};
}
// tray_denoise_halves_device's: call_rules, then its block list against the frame's number of 32 x 16 blocks
inline Refusal halves_rules(uint32_t width, uint32_t height, const Frame& f, const Params& p, const uint32_t* blocks, uint32_t n_blocks, uint32_t frame_blocks,
                            const float* fa, const float* fb, const void* scratch) {
    const std::string who("tray_denoise_halves_device");
    if (Refusal r = call_rules(who, 0u, width, height, f, Neighbours{}, p, nullptr, {fa, fb, scratch},
                               "the two films, the two outputs and the scratch buffer must be five different buffers, 16-byte aligned");
        r.rc != TRAY_OK)
        return r;
    if (blocks && n_blocks > frame_blocks) return {TRAY_E_INVALID, who + ": the block list is longer than the frame has blocks"};
    return {TRAY_OK, ""};
}
// every other call's: call_rules with what the call is and its sentence
inline Refusal guided_rules(uint32_t w, uint32_t h, const Frame& f, const Params& p, const float* out, const void* scratch) {
    return call_rules("tray_denoise_guided_device", kGuide | kGuideMayAlias, w, h, f, Neighbours{}, p, nullptr, {out, scratch},
                      "the two films must differ, the two guide films must differ, the output and the scratch buffer must differ from all four "
                      "and from each other, and all six must be 16-byte aligned");
}
inline Refusal two_pass_rules(uint32_t w, uint32_t h, const Frame& f, const Params& p, const Params& second, const float* out, const void* scratch) {
    return call_rules("tray_denoise_two_pass_device", 0u, w, h, f, Neighbours{}, p, &second, {out, scratch},
                      "the two films, the output and the scratch buffer must be four different buffers, 16-byte aligned");
}
inline Refusal demodulated_rules(uint32_t w, uint32_t h, const Frame& f, const Params& p, const Params* second, const float* out, const void* scratch) {
    return call_rules("tray_denoise_demodulated_device", kAlbedo, w, h, f, Neighbours{}, p, second, {out, scratch},
                      "the two films, the albedo film, the output and the scratch buffer must be five different buffers, 16-byte aligned");
}
inline Refusal temporal_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const float* out, const void* scratch) {
    return call_rules("tray_denoise_temporal_device", kTemporal, w, h, f, nb, p, nullptr, {out, scratch},
                      "every frame's two films, the output and the scratch buffer must be different buffers, 16-byte aligned");
}
inline Refusal temporal_demodulated_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const float* out, const void* scratch) {
    return call_rules("tray_denoise_temporal_demodulated_device", kTemporal | kAlbedo, w, h, f, nb, p, nullptr, {out, scratch},
                      "every frame's two films and albedo film, the output and the scratch buffer must be different buffers, 16-byte aligned");
}
inline Refusal temporal_halves_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const float* fa, const float* fb,
                                     const void* scratch) {
    return call_rules("tray_denoise_temporal_halves_device", kTemporal, w, h, f, nb, p, nullptr, {fa, fb, scratch},
                      "every frame's two films, the two outputs and the scratch buffer must be different buffers, 16-byte aligned");
}
inline Refusal temporal_guided_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const float* out, const void* scratch) {
    return call_rules("tray_denoise_temporal_guided_device", kTemporal | kGuide | kGuideMayAlias, w, h, f, nb, p, nullptr, {out, scratch},
                      "a frame's two films must differ, its two guide films must differ, the output and the scratch buffer must differ from every "
                      "film and from each other, and all must be 16-byte aligned");
}
inline Refusal temporal_two_pass_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const Params& second, const float* out,
                                       const void* scratch) {
    return call_rules("tray_denoise_temporal_two_pass_device", kTemporal, w, h, f, nb, p, &second, {out, scratch},
                      "every frame's two films, the output and the scratch buffer must be different buffers, 16-byte aligned");
}
// (the three demodulated two-pass temporal calls share one sentence; their guides are demodulated films of their own: all different)
constexpr const char* kDemodulatedDiffer = "every frame's films and albedo film, the outputs and the scratch buffer must be different buffers, 16-byte aligned";
inline Refusal temporal_demodulated_halves_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const float* fa, const float* fb,
                                                 const void* scratch) {
    return call_rules("tray_denoise_temporal_demodulated_halves_device", kTemporal | kAlbedo, w, h, f, nb, p, nullptr, {fa, fb, scratch}, kDemodulatedDiffer);
}
inline Refusal temporal_demodulated_guided_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const float* out,
                                                 const void* scratch) {
    return call_rules("tray_denoise_temporal_demodulated_guided_device", kTemporal | kAlbedo | kGuide, w, h, f, nb, p, nullptr, {out, scratch}, kDemodulatedDiffer);
}
inline Refusal temporal_demodulated_two_pass_rules(uint32_t w, uint32_t h, const Frame& f, const Neighbours& nb, const Params& p, const Params& second,
                                                   const float* out, const void* scratch) {
    return call_rules("tray_denoise_temporal_demodulated_two_pass_device", kTemporal | kAlbedo, w, h, f, nb, p, &second, {out, scratch}, kDemodulatedDiffer);
}

// ---- layouts: a call's scratch regions as byte offsets from the scratch base, packed in the order of the struct's members, and their total. All
// arithmetic in 64 bits: a 65535 x 65535 frame does not wrap.

struct Region { uint64_t offset, bytes; };
inline void* at(void* scratch, const Region& r) { return static_cast<char*>(scratch) + r.offset; }
inline float* film_at(void* scratch, const Region& r) { return reinterpret_cast<float*>(at(scratch, r)); }

enum : uint32_t {       // bytes per pixel of
    kRecordBytes = 48u,   // a frame's records A4, B4, V4 (denoise_kernels.h)
    kFilmBytes = 16u,     // an RGBW film
    kSumBytes = 32u,      // the sums a temporal call carries from pass to pass (temporal_kernels.h)
};
struct Packer {   // regions one behind the other
    uint64_t pixels, end;
    Packer(uint32_t width, uint32_t height) : pixels((uint64_t)width * height), end(0u) {}
    Region take(uint32_t bytes_per_pixel) { const Region r{end, pixels * bytes_per_pixel}; end += r.bytes; return r; }
};

// tray_denoise_device, tray_denoise_halves_device: 48 bytes per pixel
struct PlainLayout { Region records; uint64_t total; };
inline PlainLayout plain_layout(uint32_t width, uint32_t height) { Packer s(width, height); return {s.take(kRecordBytes), s.end}; }
// tray_denoise_temporal_device, _temporal_demodulated_device, _temporal_halves_device, _temporal_demodulated_halves_device: 128 bytes per pixel
struct TemporalLayout { Region centre, neighbour, sums; uint64_t total; };
inline TemporalLayout temporal_layout(uint32_t width, uint32_t height) {
    Packer s(width, height);
    return {s.take(kRecordBytes), s.take(kRecordBytes), s.take(kSumBytes), s.end};
}
// tray_denoise_guided_device: 96 bytes per pixel
struct GuidedLayout { Region values, guide; uint64_t total; };
inline GuidedLayout guided_layout(uint32_t width, uint32_t height) { Packer s(width, height); return {s.take(kRecordBytes), s.take(kRecordBytes), s.end}; }
// tray_denoise_two_pass_device: 128 bytes per pixel; the films' records are the first pass's scratch and the second pass's values
struct TwoPassLayout { Region values, fa, fb, guide; uint64_t total; };
inline TwoPassLayout two_pass_layout(uint32_t width, uint32_t height) {
    Packer s(width, height);
    return {s.take(kRecordBytes), s.take(kFilmBytes), s.take(kFilmBytes), s.take(kRecordBytes), s.end};
}
// tray_denoise_demodulated_device: [the filter's scratch (one pass: plain_layout, two: two_pass_layout) | E' | O'], 80 or 160 bytes per pixel
struct DemodulatedLayout { Region filter, even, odd; uint64_t total; };
inline DemodulatedLayout demodulated_layout(uint32_t width, uint32_t height, bool two_passes) {
    Packer s(width, height);
    return {s.take((uint32_t)(two_passes ? two_pass_layout(1u, 1u).total : plain_layout(1u, 1u).total)), s.take(kFilmBytes), s.take(kFilmBytes), s.end};
}
// tray_denoise_temporal_guided_device, _temporal_demodulated_guided_device: 176 bytes per pixel
struct TemporalGuidedLayout { Region centre_guide, guide, values, sums; uint64_t total; };
inline TemporalGuidedLayout temporal_guided_layout(uint32_t width, uint32_t height) {
    Packer s(width, height);
    return {s.take(kRecordBytes), s.take(kRecordBytes), s.take(kRecordBytes), s.take(kSumBytes), s.end};
}
// tray_denoise_temporal_two_pass_device, _temporal_demodulated_two_pass_device: 256 bytes per pixel; the first three regions are temporal_layout's
struct TemporalTwoPassLayout { Region centre, neighbour, sums, fa, fb, centre_guide, guide; uint64_t total; };
inline TemporalTwoPassLayout temporal_two_pass_layout(uint32_t width, uint32_t height) {
    Packer s(width, height);
    return {s.take(kRecordBytes), s.take(kRecordBytes), s.take(kSumBytes), s.take(kFilmBytes), s.take(kFilmBytes), s.take(kRecordBytes), s.take(kRecordBytes), s.end};
}

// ---- launch counts. prepare: 2 (k_dn_prepare<0>, <1>, or k_tdm_prepare and k_dn_prepare<1>); denoise: prepare and the filter; every other group: 1.
constexpr uint32_t kPrepareLaunches = 2u;
constexpr uint32_t kDenoiseLaunches = kPrepareLaunches + 1u;
constexpr uint32_t kGuidedLaunches = 2u * kPrepareLaunches + 1u;    // prepare of the values, of the guide, the guided filter
constexpr uint32_t kTwoPassLaunches = 2u * kPrepareLaunches + 2u;   // prepare of the films, the halves, prepare of the pilot, the guided filter
constexpr uint32_t kDemodLaunches = 2u;                             // demodulate before the filter, remodulate after
// The temporal calls with N neighbours. Halves (and the one-output temporal calls): per frame prepare's two and one pass. Guided: per frame prepare of
// the values, prepare of the guide, one pass. Two-pass: the halves call; prepare of the centre's pilot and the centre's guided pass; per neighbour
// prepare of its films, its own halves, prepare of its pilot, its guided pass.
constexpr uint32_t halves_launches(uint32_t n) { return (kPrepareLaunches + 1u) * (n + 1u); }
constexpr uint32_t guided_launches(uint32_t n) { return (2u * kPrepareLaunches + 1u) * (n + 1u); }
constexpr uint32_t two_pass_launches(uint32_t n) { return halves_launches(n) + kPrepareLaunches + 1u + (2u * kPrepareLaunches + 2u) * n; }
static_assert(two_pass_launches(2u) == 9u * 2u + 6u, "9 N + 6 launches: the two-pass temporal call's");

// ---- schedules. Ops has width and height and the launch groups as members (what the add-on libraries' launch functions take, without stream and size):
//   prepare(even, odd, records)                              denoise(even, odd, radius, patch, k, out, scratch)
//   halves(records, radius, patch, k, blocks, n_blocks, fa, fb)      filter(guide, values, radius, patch, k, out)
//   temporal_pass(centre, frame, radius, patch, k, sums, first, last, out)
//   tdemod_prepare(even, odd, albedo, records)               tdemod_pass(centre, frame, albedo, radius, patch, k, sums, first, last, out)
//   t2_halves_pass(centre, frame, radius, patch, k, sums, first, last, fa, fb)
//   t2_guided_pass(centre_guide, guide, values, radius, patch, k, sums, first, last, out)
//   td2_prepare(even, odd, albedo, records)                  td2_guided_pass(centre_guide, guide, values, albedo, radius, patch, k, sums, first, last, out)
//   demodulate(even, odd, albedo, even_out, odd_out)         remodulate(albedo, out)

// The frame loop of every temporal schedule: the centre's window (radius) first, then every neighbour's (radius_t) in the caller's order; the first
// pass starts the sums, the last one normalises them into the output. body(frame, radius, first, last).
template <class Body>
inline void for_each_frame(const Frame& centre, const Neighbours& nb, const Params& p, Body&& body) {
    for (uint32_t j = 0; j <= nb.n; ++j) body(j ? nb[j - 1u] : centre, j ? p.radius_t : p.radius, j == 0u, j == nb.n);
}

// tray_denoise_device: three launches
template <class Ops>
inline void denoise(Ops& ops, const Frame& f, const Params& p, float* out, void* scratch) {
    ops.denoise(f.even, f.odd, p.radius, p.patch, p.k, out, at(scratch, plain_layout(ops.width, ops.height).records));
}
// tray_denoise_halves_device: prepare and the halves over the block list (null: every block); an empty list is nothing to compute: no launch at all
template <class Ops>
inline void halves(Ops& ops, const Frame& f, const Params& p, const uint32_t* blocks, uint32_t n_blocks, float* fa, float* fb, void* scratch) {
    if (blocks && n_blocks == 0u) return;
    void* const records = at(scratch, plain_layout(ops.width, ops.height).records);
    ops.prepare(f.even, f.odd, records);
    ops.halves(records, p.radius, p.patch, p.k, blocks, n_blocks, fa, fb);
}
// tray_denoise_guided_device: five launches
template <class Ops>
inline void guided(Ops& ops, const Frame& f, const Params& p, float* out, void* scratch) {
    const GuidedLayout l = guided_layout(ops.width, ops.height);
    ops.prepare(f.even, f.odd, at(scratch, l.values));
    ops.prepare(f.guide_a, f.guide_b, at(scratch, l.guide));
    ops.filter(at(scratch, l.guide), at(scratch, l.values), p.radius, p.patch, p.k, out);
}
// tray_denoise_two_pass_device: six launches -- the first pass as tray_denoise_halves_device over every block (its records of the films are the
// second pass's values), then the guided filter with the pilot as guide
template <class Ops>
inline void two_pass(Ops& ops, const Frame& f, const Params& p, const Params& second, float* out, void* scratch) {
    const TwoPassLayout l = two_pass_layout(ops.width, ops.height);
    float* const fa = film_at(scratch, l.fa), * const fb = film_at(scratch, l.fb);
    ops.prepare(f.even, f.odd, at(scratch, l.values));
    ops.halves(at(scratch, l.values), p.radius, p.patch, p.k, nullptr, 0u, fa, fb);
    ops.prepare(fa, fb, at(scratch, l.guide));
    ops.filter(at(scratch, l.guide), at(scratch, l.values), second.radius, second.patch, second.k, out);
}
// tray_denoise_demodulated_device: the one-pass (second == null) or two-pass filter of E' and O', between demodulate and remodulate
template <class Ops>
inline void demodulated(Ops& ops, const Frame& f, const Params& p, const Params* second, float* out, void* scratch) {
    const DemodulatedLayout l = demodulated_layout(ops.width, ops.height, second != nullptr);
    const Frame quotients{film_at(scratch, l.even), film_at(scratch, l.odd), nullptr, nullptr, nullptr};
    ops.demodulate(f.even, f.odd, f.albedo, film_at(scratch, l.even), film_at(scratch, l.odd));
    if (second) two_pass(ops, quotients, p, *second, out, at(scratch, l.filter));
    else denoise(ops, quotients, p, out, at(scratch, l.filter));
    ops.remodulate(f.albedo, out);
}
// tray_denoise_temporal_device / _temporal_demodulated_device: 3 (N + 1) launches -- per frame its records (through its albedo) and one pass; the
// demodulated call's last pass scales the output by the centre's albedo
template <bool kDemodulated = false, class Ops>
inline void temporal(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* out, void* scratch) {
    const TemporalLayout l = temporal_layout(ops.width, ops.height);
    void* const c = at(scratch, l.centre), * const sums = at(scratch, l.sums);
    for_each_frame(centre, nb, p, [&](const Frame& f, uint32_t radius, bool first, bool last) {
        void* const records = first ? c : at(scratch, l.neighbour);
        if constexpr (kDemodulated) {
            ops.tdemod_prepare(f.even, f.odd, f.albedo, records);
            ops.tdemod_pass(c, records, centre.albedo, radius, p.patch, p.k, sums, first, last, out);
        } else {
            ops.prepare(f.even, f.odd, records);
            ops.temporal_pass(c, records, radius, p.patch, p.k, sums, first, last, out);
        }
    });
}
template <class Ops>
inline void temporal_demodulated(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* out, void* scratch) {
    temporal<true>(ops, centre, nb, p, out, scratch);
}
// the 3 (N + 1) launches of the pilot over all frames into (fa, fb), in the three regions of a temporal_layout; l.centre keeps the centre's records
template <bool kDemodulated, class Ops>
inline void pilot_over_frames(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* fa, float* fb, void* scratch,
                              const TemporalLayout& l) {
    void* const c = at(scratch, l.centre), * const sums = at(scratch, l.sums);
    for_each_frame(centre, nb, p, [&](const Frame& f, uint32_t radius, bool first, bool last) {
        void* const records = first ? c : at(scratch, l.neighbour);
        if constexpr (kDemodulated) ops.td2_prepare(f.even, f.odd, f.albedo, records);
        else ops.prepare(f.even, f.odd, records);
        ops.t2_halves_pass(c, records, radius, p.patch, p.k, sums, first, last, fa, fb);
    });
}
// tray_denoise_temporal_halves_device / _temporal_demodulated_halves_device: that pilot
template <bool kDemodulated = false, class Ops>
inline void temporal_halves(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* fa, float* fb, void* scratch) {
    pilot_over_frames<kDemodulated>(ops, centre, nb, p, fa, fb, scratch, temporal_layout(ops.width, ops.height));
}
template <class Ops>
inline void temporal_demodulated_halves(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* fa, float* fb, void* scratch) {
    temporal_halves<true>(ops, centre, nb, p, fa, fb, scratch);
}
// one guided pass of the two calls below: td2_guided_pass scales the last pass's output by the centre's albedo
template <bool kDemodulated, class Ops>
inline void guided_pass(Ops& ops, const void* centre_guide, const void* guide, const void* values, const float* albedo, uint32_t radius, const Params& p,
                        void* sums, bool first, bool last, float* out) {
    if constexpr (kDemodulated) ops.td2_guided_pass(centre_guide, guide, values, albedo, radius, p.patch, p.k, sums, first, last, out);
    else ops.t2_guided_pass(centre_guide, guide, values, radius, p.patch, p.k, sums, first, last, out);
}
// tray_denoise_temporal_guided_device / _temporal_demodulated_guided_device: 5 (N + 1) launches -- per frame prepare of the (demodulated) values,
// prepare of the guide, one pass
template <bool kDemodulated = false, class Ops>
inline void temporal_guided(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* out, void* scratch) {
    const TemporalGuidedLayout l = temporal_guided_layout(ops.width, ops.height);
    void* const cg = at(scratch, l.centre_guide), * const values = at(scratch, l.values);
    for_each_frame(centre, nb, p, [&](const Frame& f, uint32_t radius, bool first, bool last) {
        void* const guide = first ? cg : at(scratch, l.guide);
        if constexpr (kDemodulated) ops.td2_prepare(f.even, f.odd, f.albedo, values);
        else ops.prepare(f.even, f.odd, values);
        ops.prepare(f.guide_a, f.guide_b, guide);
        guided_pass<kDemodulated>(ops, cg, guide, values, centre.albedo, radius, p, at(scratch, l.sums), first, last, out);
    });
}
template <class Ops>
inline void temporal_demodulated_guided(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, float* out, void* scratch) {
    temporal_guided<true>(ops, centre, nb, p, out, scratch);
}
// tray_denoise_temporal_two_pass_device / _temporal_demodulated_two_pass_device: 9 N + 6 launches. First pass: the centre's pilot over all frames.
// Second pass: the centre (its records are still in l.centre) guided by that pilot, then every neighbour guided by its own single-frame pilot, one at
// a time -- its records are resolved again (the first pass's are overwritten by the next neighbour's), and (fa, fb) is free once the pilot before it
// is resolved. The pilots are (demodulated) films already: prepare takes them as they are.
template <bool kDemodulated = false, class Ops>
inline void temporal_two_pass(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, const Params& second, float* out, void* scratch) {
    const TemporalTwoPassLayout l = temporal_two_pass_layout(ops.width, ops.height);
    float* const fa = film_at(scratch, l.fa), * const fb = film_at(scratch, l.fb);
    void* const cg = at(scratch, l.centre_guide);
    pilot_over_frames<kDemodulated>(ops, centre, nb, p, fa, fb, scratch, TemporalLayout{l.centre, l.neighbour, l.sums, 0u});
    for_each_frame(centre, nb, second, [&](const Frame& f, uint32_t radius, bool first, bool last) {
        void* const values = first ? at(scratch, l.centre) : at(scratch, l.neighbour);
        if (!first) {
            if constexpr (kDemodulated) ops.td2_prepare(f.even, f.odd, f.albedo, values);
            else ops.prepare(f.even, f.odd, values);
            ops.halves(values, p.radius, p.patch, p.k, nullptr, 0u, fa, fb);
        }
        void* const guide = first ? cg : at(scratch, l.guide);
        ops.prepare(fa, fb, guide);
        guided_pass<kDemodulated>(ops, cg, guide, values, centre.albedo, radius, second, at(scratch, l.sums), first, last, out);
    });
}
template <class Ops>
inline void temporal_demodulated_two_pass(Ops& ops, const Frame& centre, const Neighbours& nb, const Params& p, const Params& second, float* out, void* scratch) {
    temporal_two_pass<true>(ops, centre, nb, p, second, out, scratch);
}

}  // namespace tr_dnplan
