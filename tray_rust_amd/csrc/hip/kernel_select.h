// Which instantiation of k_path_tiles / k_sampler_pass a scene runs: one selector per kernel family, for every launch site -- device_api.hip (the
// whole-frame launch and the occupancy query), kernel_ranges.hip (the sample-range launch) and the host emulation (tests/emu). A selector calls
// f(kernel) with the chosen instantiation; f supplies the arguments, so the same selector serves with and without the range parameters of
// TR_SAMPLE_RANGES builds (a function pointer carries no default arguments: pass them all). The instantiations named here are exactly those of
// kernel_list.h / kernel_ranges.hip; where the kernels are only declared (TR_INST_EXTERN), include that list first.
#pragma once

// ANIM is the caller's choice (`anim ? select_path_tiles<1>(..) : select_path_tiles<0>(..)`): a translation unit that names one ANIM instantiates only its kernels
// (kernel_ranges.hip's groups). The Whitted integrator has one instantiation per ANIM; light_filter: the form with mis_ray_filter (tray_scene_create).
template <int ANIM, int FEAT, class F>
void select_path_tiles_filter(bool light_filter, F&& f) {
    if (light_filter) f(k_path_tiles<ANIM, FEAT, TRAY_INTEGRATOR_PATH, true>); else f(k_path_tiles<ANIM, FEAT, TRAY_INTEGRATOR_PATH, false>);
}
template <int ANIM, class F>
void select_path_tiles(int feat, bool whitted, bool light_filter, F&& f) {
    if (whitted) f(k_path_tiles<ANIM, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_WHITTED>);
    else if (feat == FEAT_NONE) select_path_tiles_filter<ANIM, FEAT_NONE>(light_filter, f);
    else if (feat == FEAT_MERL) select_path_tiles_filter<ANIM, FEAT_MERL>(light_filter, f);
    else if (feat == FEAT_SPEC) select_path_tiles_filter<ANIM, FEAT_SPEC>(light_filter, f);
    else if (feat == (FEAT_MERL | FEAT_SPEC)) select_path_tiles_filter<ANIM, FEAT_MERL | FEAT_SPEC>(light_filter, f);
    else if (feat == (FEAT_ALL | FEAT_TEX)) select_path_tiles_filter<ANIM, FEAT_ALL | FEAT_TEX>(light_filter, f);
    else select_path_tiles_filter<ANIM, FEAT_ALL>(light_filter, f);
}

// k_sampler_pass; anim: 0 static, 2 moving, 3 a scene with an AnimatedMesh
inline bool sampler_lean(int feat, uint32_t integrator) { return feat == FEAT_NONE && integrator != TRAY_INTEGRATOR_WHITTED; }   // (no optional lobe, no texture: the small instantiation)
template <class F>
void select_sampler_pass(int anim, bool lean, F&& f) {
    if (anim == 3) { if (lean) f(k_sampler_pass<3, FEAT_NONE>); else f(k_sampler_pass<3, FEAT_ALL | FEAT_TEX>); }
    else if (anim == 2) { if (lean) f(k_sampler_pass<2, FEAT_NONE>); else f(k_sampler_pass<2, FEAT_ALL | FEAT_TEX>); }
    else { if (lean) f(k_sampler_pass<0, FEAT_NONE>); else f(k_sampler_pass<0, FEAT_ALL | FEAT_TEX>); }
}
