// ptx_render_nee in one launch per pass under active motion (PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION): k_nee_fused's loop (nee_fused.hip) with a
// time per lane. A lane that starts sample `id` computes the sample's time u (sample_time) and keeps it for the whole path: the camera ray
// comes from the camera at u, every ray of the path (closest hit, sun, light) is traced through scene_traverse_motion at u, and a vertex on a
// moving model takes its attributes from the model's records at u — what k_nee_generate, k_intersect_batch_motion and k_nee_shade do in the
// record-based form, in the same arithmetic. So the frame and the stats are bitwise those of the unflagged call under the same motion
// (include/ptx.h: MOTION), as k_nee_fused's are without motion.
// Which statements run is decided by the kernel argument Mo, wave-uniformly: with the camera alone moving the motion table is not read and
// the static scene_traverse runs; with models alone moving the camera is the scene's.
// A translation unit of its own: nee_fused.hip and its kernels are not touched by motion.
// Numerics as in kernels.hip: IEEE binary32 in the written order, no contraction.
#include "nee_core.hpp"

namespace ptx {

// Threads per workgroup of a variant, by nee_fused_block's rule: the largest of 768, 512 and 256 at which every mode of the variant compiles
// WITHOUT scratch. Besides k_nee_fused's state a lane holds u for the whole path, basis(u) across the walks of a moving space (9 VGPRs) and
// the 33 floats of XformRecs around hit_attributes_at. No variant fits 768 threads (168 VGPRs): the four that run there without motion
// (no texture, sun, ENV, RIS or PUN code) spill 34-41 VGPRs and get 512 (200-204 VGPRs). At 512 threads (256 VGPRs) the variants with ENV
// and SUN code together spill 2-36 VGPRs, and the RIS variants with texture code and SUN or ENV code 2-39: those 32 get 256 threads
// (256 VGPRs and 2-35 AGPRs). The other 64 run with 512 threads (200-256 VGPRs). All 288 kernels were compiled; none uses scratch
// (DESIGN.md 5.12 has the table).
// -DPTX_NEE_FUSED_MOTION_BLOCK=n: one size for all (measurement).
constexpr int nee_fused_motion_block(uint32_t V) {
#ifdef PTX_NEE_FUSED_MOTION_BLOCK
	return PTX_NEE_FUSED_MOTION_BLOCK;
#else
	const bool tex = (V & NEE_TEX) != 0, sun = (V & NEE_SUN) != 0, env = (V & NEE_ENV) != 0, ris = (V & NEE_RIS) != 0;
	return (env && sun) || (ris && tex && (sun || env)) ? 256 : 512;
#endif
}
constexpr bool nee_fused_motion_block_fits(uint32_t V) { return nee_fused_motion_block(V) % 64 == 0 && nee_fused_motion_block(V) <= kBlock; }
static_assert(nee_all_variants(nee_fused_motion_block_fits), "whole waves, and the spill area is sized for kBlock / 64 waves per workgroup");

DEV uint32_t wave_sum_motion(uint32_t v) {
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
	return v;   // lane 0 holds the sum
}

// the closest hit of a ray of time u: with no model moving (a kernel argument: wave-uniform) the static traversal, and the table is not read
template <int MODE>
DEV bool traverse_at(const DevScene& S, const RenderMotion& Mo, const Geoms& g, V3 o, V3 d, float u, SceneHit& h, const Spill& spill) {
	if (Mo.models_moved) return scene_traverse_motion<MODE>(S, Mo.models, g, o, d, u, h, spill);
	return scene_traverse<MODE>(S, g, o, d, h, spill);
}

// V: the variant (nee_core.hpp has the bits), as for k_nee_fused. Mo0: the scene's motion (active); its table's pointers come a second time
// as arguments of their own (t_begin, t_end, t_moved), scalar-loaded like the scene's tables.
template <int MODE, uint32_t V>
__global__ void __launch_bounds__(nee_fused_motion_block(V)) k_nee_fused_motion(DevScene S0, RenderParams P, NeeLights Lt, NeeFusedBuffers B, const ModelRec* __restrict__ t_models,
                                                                            const SurfaceRec* __restrict__ t_surfaces, const SpaceRec* __restrict__ t_spaces,
                                                                            const uint32_t* __restrict__ t_model_space, NeeEnv Ev, uint32_t ris_m, NeePunctual Pn, RenderMotion Mo0,
                                                                            const float* __restrict__ t_begin, const float* __restrict__ t_end, const uint32_t* __restrict__ t_moved) {
	constexpr bool SUN = (V & NEE_SUN) != 0, ENV = (V & NEE_ENV) != 0, PUN = (V & NEE_PUN) != 0;
	constexpr int kThreads = nee_fused_motion_block(V);
	DevScene S = S0;
	S.models = t_models; S.surfaces = t_surfaces; S.spaces = t_spaces; S.model_space = t_model_space;  // see struct Tables
	RenderMotion Mo = Mo0;
	Mo.models.begin_xform = t_begin; Mo.models.end_xform = t_end; Mo.models.moved = t_moved;
	const Staged st = stage_geometry<MODE>(S, g_smem);
	// S.hot_lds stays unset, as in k_nee_fused
	const Geoms g = st.g;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave_slot = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
	const Spill spill{B.spill + (size_t)wave_slot * (kSpillStack * 64) + lane};
	uint32_t rays = 0, light_samples = 0, light_visible = 0;   // of this lane

	// wave-uniform: the chunk's ids [chunk_first + cursor, chunk_first + chunk_n) are unstarted; dry = the pass has no chunk left
	uint32_t chunk_first = 0, chunk_n = 0, cursor = 0;
	bool dry = false;
	// the lane's path
	bool have = false;
	uint32_t id = 0, pixel = 0, sample = 0, depth = 0, pass = 0;
	V3 o = {0, 0, 0}, d = {0, 0, 1}, T = {1, 1, 1}, L = {0, 0, 0};
	float p_prev = 0;
	float u = 0;   // the path's time

	for (;;) {
		// ---------------- idle lanes take the next unstarted ids
		for (;;) {
			const uint64_t idle = __ballot(!have);
			if (idle == 0 || dry) break;
			if (cursor == chunk_n) {
				// Guided self-scheduling (k_render_pass): full chunks while plenty of paths are left, then chunks that shrink with what remains
				uint32_t first_lo = 0, first_hi = 0, take = 0;
				if (lane == 0) {
					const unsigned long long seen = __hip_atomic_load(B.chunk_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					const unsigned long long left = seen < P.n_paths ? P.n_paths - seen : 0ull;
					const unsigned long long n_waves = (unsigned long long)gridDim.x * (kThreads / 64);
					unsigned long long want = P.n_paths >= 16ull * n_waves * kChunk ? (unsigned long long)kChunk : left / n_waves;
					want = (want + 63ull) & ~63ull;
					take = (uint32_t)(want < 128ull ? 128ull : (want > (unsigned long long)kChunk ? (unsigned long long)kChunk : want));
					const unsigned long long f = atomicAdd(B.chunk_counter, (unsigned long long)take);
					first_lo = (uint32_t)f; first_hi = (uint32_t)(f >> 32);
				}
				first_lo = __builtin_amdgcn_readfirstlane(first_lo);
				first_hi = __builtin_amdgcn_readfirstlane(first_hi);
				take = __builtin_amdgcn_readfirstlane(take);
				const uint64_t first = ((uint64_t)first_hi << 32) | first_lo;
				if (first >= P.n_paths) { dry = true; break; }
				chunk_first = (uint32_t)first;
				chunk_n = (uint32_t)((P.n_paths - first) < (uint64_t)take ? (P.n_paths - first) : take);
				cursor = 0;
				if (P.bounces == 0) {   // trace(0, ..) is black with alpha 1 (renderer.cpp:438-439): no vertex ever runs
					for (uint32_t i = lane; i < chunk_n; i += 64) B.sample_rad[chunk_first + i] = make_float4(0.f, 0.f, 0.f, 1.0f);
					cursor = chunk_n;
					continue;
				}
			}
			const uint32_t avail = chunk_n - cursor, n_idle = (uint32_t)__popcll(idle);
			const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));   // idle lanes below this one
			if (!have && rank < avail) {
				id = chunk_first + cursor + rank;
				uint32_t px, py;
				nee_sample_of(P, id, px, py, sample);
				pixel = py * P.W + px;
				u = sample_time(P, Mo, pixel, sample);
				if (Mo.camera_moved) {
					// the camera of the lane's own time: S is wave-uniform and u is not, so the blend goes into a copy that lives in this branch alone
					DevScene Sc = S;
					camera_at(Sc, Mo, u);
					camera_ray(Sc, P, px, py, sample, o, d);
				} else {
					camera_ray(S, P, px, py, sample, o, d);
				}
				T = mk(1.0f, 1.0f, 1.0f); L = mk(0.f, 0.f, 0.f);
				p_prev = 0.0f; depth = 0; pass = 0;
				have = true;
			}
			cursor += n_idle < avail ? n_idle : avail;
		}
		if (__ballot(have) == 0) break;   // dry, and every path of the wave has ended

		if (have) {
			// ---------------- closest hit at the path's time, as the intersect route reports it (write_hit_outputs_motion)
			SceneHit h;
			const bool hit = traverse_at<MODE>(S, Mo, g, o, d, u, h, spill);
			rays++;
			const int32_t surf = hit ? h.surface : -1;
			const uint32_t tri = hit ? (h.tri & S.tri_id_mask) - S.surfaces[h.surface].tri_base : 0u;
			bool moved = false;
			XformRecs Xm;
			if (Mo.models_moved && hit) {
				const uint32_t m = S.surfaces[h.surface].model;
				moved = Mo.models.moved[m] != 0u;
				if (moved) model_records_at(Mo.models, m, u, Xm);   // the hit surface's records at the path's time, as in k_nee_shade
			}
			NeeVertex v;
			nee_vertex<V>(S, P, Lt, Ev, ris_m, pixel, sample, surf, tri, hit ? h.b1 : 0.f, hit ? h.b2 : 0.f, hit ? h.dist : -1.0f, o, d, T, L, p_prev, depth, pass, v, Pn, moved, Xm);
			bool alive = v.alive;
			// ---------------- the sun ray: occluded = any hit
			if constexpr (SUN) {
				if (v.want_sun) {
					SceneHit sh;
					const bool occluded = traverse_at<MODE>(S, Mo, g, v.sun_o, v.sun_d, u, sh, spill);
					rays++;
					if (v.catcher_req) {
						// lit catcher = fully transparent: same depth, next pass (the vertex left the path state as it found it); shadowed: the path ends with what it has
						if (!occluded && pass + 1u <= 4096u) {
							o = v.sun_x;
							d = normalize(d);
							pass++;
							alive = true;
						}
					} else if (!occluded) {
						L.x += v.sun_x.x; L.y += v.sun_x.y; L.z += v.sun_x.z;
					}
				}
			}
			// ---------------- the light ray: visible = its closest hit is the sampled triangle
			if (v.want_light) {
				SceneHit lh;
				const bool lhit = traverse_at<MODE>(S, Mo, g, v.lo, v.ld, u, lh, spill);
				rays++;
				light_samples++;
				bool visible;
				if (PUN && v.exp_surf == kNeePunctualRay) visible = !lhit || !(lh.dist < __uint_as_float(v.exp_tri));   // a punctual sample: nothing nearer than the light
				else if (ENV && v.exp_surf == kNeeEnvRay) visible = !lhit;   // an environment sample
				else visible = lhit && lh.surface == (int32_t)v.exp_surf && (int32_t)((lh.tri & S.tri_id_mask) - S.surfaces[lh.surface].tri_base) == (int32_t)v.exp_tri;
				if (visible) {
					light_visible++;
					L.x += v.lx.x; L.y += v.lx.y; L.z += v.lx.z;
				}
			}
			if (!alive) {
				B.sample_rad[id] = make_float4(L.x, L.y, L.z, 1.0f);
				have = false;
			}
		}
	}

	// the wave has run dry: its counts, one vector atomic per counter
	const uint32_t r = wave_sum_motion(rays), ls = wave_sum_motion(light_samples), lv = wave_sum_motion(light_visible);
	if (lane == 0) {
		if (r) atomicAdd(B.counters, (unsigned long long)r);
		if (ls) atomicAdd(B.counters + 1, (unsigned long long)ls);
		if (lv) atomicAdd(B.counters + 2, (unsigned long long)lv);
	}
}

// ------------------------------------------------------------------------------------ launcher
// This file is compiled once per part (nee_core.hpp: the SPDF, RIS and PUN bits of the mask), with -DPTX_NEE_PART=<part>, as nee_fused.hip is:
// each compilation holds the 36 kernels of its part and defines launch_nee_fused_motion_part<its part>; part 0 holds launch_nee_fused_motion
// as well, which picks the part by the mask's high bits.
#ifndef PTX_NEE_PART
#error "nee_fused_motion.hip is compiled once per part of the variants: -DPTX_NEE_PART=<0..7> (the Makefile's NEE_FUSED_MOTION_PARTS)"
#endif
static_assert(PTX_NEE_PART >= 0 && PTX_NEE_PART < (int)kNeeParts, "a part is the SPDF, RIS and PUN bits of a variant");

using NeeFusedMotionKernel = decltype(&k_nee_fused_motion<MODE_GLOBAL, 0u>);
struct NeeFusedMotionTable { NeeFusedMotionKernel fn[kNeeSceneMask + 1]; };   // by the low four bits; nullptr: no such variant

// the kernels of MODE in this part: one entry for every mask of kNeeVariants that lies in it
template <int MODE, size_t... I>
static NeeFusedMotionTable nee_fused_motion_table(std::index_sequence<I...>) {
	NeeFusedMotionTable t{};
	([&] {
		constexpr uint32_t V = kNeeVariants.v[I];
		if constexpr ((V >> kNeePartShift) == PTX_NEE_PART) t.fn[V & kNeeSceneMask] = &k_nee_fused_motion<MODE, V>;
	}(), ...);
	return t;
}

template <int MODE>
static hipError_t launch_nee_fused_motion_mode(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const RenderMotion& Mo,
                                               const NeeFusedBuffers& B, size_t lds_bytes, int grid, hipStream_t stream) {
	static const NeeFusedMotionTable table = nee_fused_motion_table<MODE>(std::make_index_sequence<kNeeVariantCount>{});
	const NeeFusedMotionKernel kernel = table.fn[V & kNeeSceneMask];
	if (!kernel) return hipErrorInvalidValue;
	if (MODE != MODE_GLOBAL) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(nee_fused_motion_block(V)), MODE != MODE_GLOBAL ? lds_bytes : 0, stream, S, P, Lt, B, S.models, S.surfaces, S.spaces, S.model_space, Ev, ris_m, Pn, Mo,
	                   Mo.models.begin_xform, Mo.models.end_xform, Mo.models.moved);
	return hipGetLastError();
}

// Declared for every part, defined by the one compilation of that part, as an explicit specialisation of a template without a body
// (nee_fused.hip has the reason): the linker puts the eight together.
template <uint32_t PART>
hipError_t launch_nee_fused_motion_part(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const RenderMotion& Mo,
                                        const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream);
template <>
hipError_t launch_nee_fused_motion_part<PTX_NEE_PART>(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m,
                                                      const RenderMotion& Mo, const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	if (mode == MODE_LDS) return launch_nee_fused_motion_mode<MODE_LDS>(V, S, P, Lt, Ev, Pn, ris_m, Mo, B, lds_bytes, grid, stream);
	if (mode == MODE_HYBRID) return launch_nee_fused_motion_mode<MODE_HYBRID>(V, S, P, Lt, Ev, Pn, ris_m, Mo, B, lds_bytes, grid, stream);
	return launch_nee_fused_motion_mode<MODE_GLOBAL>(V, S, P, Lt, Ev, Pn, ris_m, Mo, B, lds_bytes, grid, stream);
}

#if PTX_NEE_PART == 0
template <size_t... PART>
static hipError_t launch_nee_fused_motion_in_part(std::index_sequence<PART...>, uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn,
                                                  uint32_t ris_m, const RenderMotion& Mo, const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	static constexpr decltype(&launch_nee_fused_motion_part<0>) parts[] = {&launch_nee_fused_motion_part<PART>...};
	return parts[V >> kNeePartShift](V, S, P, Lt, Ev, Pn, ris_m, Mo, B, mode, lds_bytes, grid, stream);
}

// the variant: nee_select_variant (nee_core.hpp), as for launch_nee_fused. The kernel is for active motion alone, and a missing motion
// table is an error, never a static launch (launch_intersect_motion has the same rule).
hipError_t launch_nee_fused_motion(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const RenderMotion& Mo,
                                   const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	if (!Mo.active) return hipErrorInvalidValue;
	if (Mo.models_moved && (!Mo.models.begin_xform || !Mo.models.end_xform || !Mo.models.moved)) return hipErrorInvalidValue;
	uint32_t V, ris_m;
	const hipError_t e = nee_select_variant(S, Lt, Ev, Pn, sampler_pdf, candidates, V, ris_m);
	if (e == hipSuccess && (V & NEE_LTREE)) return hipErrorInvalidValue;   // no tree variants of this kernel: the host runs the unfused form in tree mode
	if (e != hipSuccess) return e;
	return launch_nee_fused_motion_in_part(std::make_index_sequence<kNeeParts>{}, V, S, P, Lt, Ev, Pn, ris_m, Mo, B, mode, lds_bytes, grid, stream);
}
#endif

}  // namespace ptx
