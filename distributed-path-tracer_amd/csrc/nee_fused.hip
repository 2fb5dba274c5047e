// ptx_render_nee in one launch per pass (PTX_NEE_FUSED): the estimator of nee.hip — the same vertex function, nee_core.hpp — without the
// host-driven rounds and their streams. Persistent workgroups, one per CU, stage the geometry as k_render_pass does; after that every LANE
// owns one path from its camera ray to its end: closest hit (scene_traverse), nee_vertex, the sun ray if the vertex asked for one, the light
// ray if it asked for one, next vertex. The path state and the sample's radiance stay in registers; the only per-sample memory is the final
// float4 (L, 1) of sample_rad[id], which k_resolve adds up as for every other renderer.
// Work: a wave takes chunks of sample ids from the pass's counter (one 64-bit atomic per chunk, guided self-scheduling as in k_render_pass);
// a lane whose path has ended takes the chunk's next unstarted id at the head of the loop (wave-uniform cursor + ballot + lane prefix
// count), so waves stay full while paths die. Everything a sample computes is keyed by its id — pixel, sample index, Philox key — so which
// lane runs it changes no bit, and L receives vertex k's emission, sun term and light term, then vertex k + 1's: the additions of the
// record-based form in its order. The frame is bitwise that of the unflagged call.
// Numerics as in kernels.hip: IEEE binary32 in the written order, no contraction.
#include "nee_core.hpp"

namespace ptx {

// Threads per workgroup (one workgroup per CU) of a variant. One vertex's registers plus a traversal do not fit the 128 VGPRs of k_render_pass's
// 1024-thread workgroup, so the kernel has launch bounds of its own: the largest workgroup at which the variant compiles WITHOUT scratch.
// 768 threads = 3 waves per SIMD = 168 VGPRs hold the variants without texture and sun code (158-165 VGPRs); the others need 174-210 and
// get 512 threads = 2 waves per SIMD = 256 VGPRs; so do the ENV variants (always TEX: 207-228 VGPRs). Occupancy is what the kernel runs on (Cornell: 256 threads 185, 512 353, 768 465 Msamples/s;
// DESIGN.md 5.7 has the resource table and the measurement). Staging is per workgroup and there is one workgroup per CU either way; the
// overflow stacks are sized per wave slot of the larger k_render_pass workgroup. The RIS variants (PTX_NEE_CANDIDATES) carry the reservoir across the
// candidate loop: those without texture and sun code spill 2 to 4 VGPRs at 768 threads and get 512 as well; the others stay without scratch at 512 (198-255 VGPRs).
// The PUN variants (punctual lights on the scene) carry the punctual branch of the candidate besides the others and get 512 threads: 166-231
// VGPRs without RIS, 184-256 with. One is too full for that: with ENV, SUN, RIS and SPDF together the global-memory variant with ALPHA spills
// 3 VGPRs at 512, so the variants of that combination get 256 (up to 260 VGPRs). All 144 were compiled; none uses scratch.
// The LTREE variants (a light tree over the light list) carry x_prev and the descent: 2 to 10 VGPRs over their twins, at their twins' sizes
// but for ENV, SUN, RIS and PUN together without SPDF, whose LDS and hybrid variants spill 1 VGPR at 512 and get 256 as well.
// -DPTX_NEE_FUSED_BLOCK=n: one size for all (measurement).
constexpr int nee_fused_block(uint32_t V) {
#ifdef PTX_NEE_FUSED_BLOCK
	return PTX_NEE_FUSED_BLOCK;
#else
	constexpr uint32_t kFullest = NEE_PUN | NEE_RIS | NEE_SPDF | NEE_ENV | NEE_SUN;
	constexpr uint32_t kFullestTree = NEE_LTREE | NEE_PUN | NEE_RIS | NEE_ENV | NEE_SUN;   // the descent and x_prev fill that combination without SPDF too
	return ((V & kFullest) == kFullest || (V & kFullestTree) == kFullestTree) ? 256 : (V & (NEE_TEX | NEE_SUN | NEE_ENV | NEE_RIS | NEE_PUN)) ? 512 : 768;
#endif
}
constexpr bool nee_fused_block_fits(uint32_t V) { return nee_fused_block(V) % 64 == 0 && nee_fused_block(V) <= kBlock; }
static_assert(nee_all_variants(nee_fused_block_fits), "whole waves, and the spill area is sized for kBlock / 64 waves per workgroup");
constexpr bool nee_fused_tree_blocks_fit() {
	for (uint32_t i = 0; i < kNeeVariantCount; i++)
		if (!nee_fused_block_fits(kNeeTreeVariants.v[i])) return false;
	return true;
}
static_assert(nee_fused_tree_blocks_fit(), "the tree variants too");

DEV uint32_t wave_sum(uint32_t v) {
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
	return v;   // lane 0 holds the sum
}

// V: the variant (nee_core.hpp has the bits).
// ENV: the variants of PTX_NEE_ENV_SAMPLES (TEX only); Ev, the last argument, is read by them alone.
// SPDF: the variants of PTX_NEE_SAMPLER_PDF. sampler_pdf costs them 0 to 2 VGPRs, and each compiles without scratch at its unflagged
// twin's workgroup size, so nee_fused_block holds for them too (DESIGN.md 5.7 has their rows).
// RIS: the variants of PTX_NEE_CANDIDATES, the light sample chosen among ris_m candidates; the other variants do not read ris_m.
// PUN: the variants for scenes with punctual lights (Pn), a third kind of candidate; the other variants do not read Pn.
// LTREE: the variants for a non-empty light list in tree mode (kNeeTreeVariants): the lane carries x_prev, three more registers, and the
// vertex descends the light tree; the other variants have neither.
template <int MODE, uint32_t V>
__global__ void __launch_bounds__(nee_fused_block(V)) k_nee_fused(DevScene S0, RenderParams P, NeeLights Lt, NeeFusedBuffers B, const ModelRec* __restrict__ t_models,
                                                              const SurfaceRec* __restrict__ t_surfaces, const SpaceRec* __restrict__ t_spaces, const uint32_t* __restrict__ t_model_space,
                                                              NeeEnv Ev, uint32_t ris_m, NeePunctual Pn) {
	constexpr bool SUN = (V & NEE_SUN) != 0, ENV = (V & NEE_ENV) != 0, PUN = (V & NEE_PUN) != 0, LTREE = (V & NEE_LTREE) != 0;
	constexpr int kThreads = nee_fused_block(V);
	DevScene S = S0;
	S.models = t_models; S.surfaces = t_surfaces; S.spaces = t_spaces; S.model_space = t_model_space;  // see struct Tables
	const Staged st = stage_geometry<MODE>(S, g_smem);
	// S.hot_lds stays unset: nee_vertex names a triangle by its index within the mesh, as the intersect route reports it, and reads its hit record from S.tris
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
	V3 x_prev = {0, 0, 0};   // LTREE alone: the position of the vertex that drew the BSDF sample; read at depth != 0 only, after that vertex set it

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
				camera_ray(S, P, px, py, sample, o, d);
				T = mk(1.0f, 1.0f, 1.0f); L = mk(0.f, 0.f, 0.f);
				p_prev = 0.0f; depth = 0; pass = 0;
				have = true;
			}
			cursor += n_idle < avail ? n_idle : avail;
		}
		if (__ballot(have) == 0) break;   // dry, and every path of the wave has ended

		if (have) {
			// ---------------- closest hit, as the intersect route reports it (write_hit_outputs)
			SceneHit h;
			const bool hit = scene_traverse<MODE>(S, g, o, d, h, spill);
			rays++;
			const int32_t surf = hit ? h.surface : -1;
			const uint32_t tri = hit ? (h.tri & S.tri_id_mask) - S.surfaces[h.surface].tri_base : 0u;
			NeeVertex v;
			nee_vertex<V>(S, P, Lt, Ev, ris_m, pixel, sample, surf, tri, hit ? h.b1 : 0.f, hit ? h.b2 : 0.f, hit ? h.dist : -1.0f, o, d, T, L, p_prev, depth, pass, v, Pn, false, XformRecs{},
			              LTREE ? &x_prev : nullptr);
			bool alive = v.alive;
			// ---------------- the sun ray: occluded = any hit
			if constexpr (SUN) {
				if (v.want_sun) {
					SceneHit sh;
					const bool occluded = scene_traverse<MODE>(S, g, v.sun_o, v.sun_d, sh, spill);
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
				const bool lhit = scene_traverse<MODE>(S, g, v.lo, v.ld, lh, spill);
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
	const uint32_t r = wave_sum(rays), ls = wave_sum(light_samples), lv = wave_sum(light_visible);
	if (lane == 0) {
		if (r) atomicAdd(B.counters, (unsigned long long)r);
		if (ls) atomicAdd(B.counters + 1, (unsigned long long)ls);
		if (lv) atomicAdd(B.counters + 2, (unsigned long long)lv);
	}
}

// ------------------------------------------------------------------------------------ launcher
static hipError_t set_lds(const void* fn, size_t bytes) {
	return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// This file is compiled once per part (nee_core.hpp: the SPDF, RIS, PUN and LTREE bits of the mask), with -DPTX_NEE_PART=<part>, so that the
// sixteen parts of the variants build side by side: parts 0 to 7 hold kNeeVariants, parts 8 to 15 the tree variants (kNeeTreeVariants). Each
// compilation holds the 36 kernels of its part and defines launch_nee_fused_part<its part>; part 0 holds launch_nee_fused as well, which
// picks the part by the mask's high bits.
#ifndef PTX_NEE_PART
#error "nee_fused.hip is compiled once per part of the variants: -DPTX_NEE_PART=<0..15> (the Makefile's NEE_FUSED_PARTS)"
#endif
constexpr uint32_t kNeeFusedParts = 2 * kNeeParts;
static_assert(PTX_NEE_PART >= 0 && PTX_NEE_PART < (int)kNeeFusedParts, "a part is the SPDF, RIS, PUN and LTREE bits of a variant");
static_assert(NEE_LTREE >> kNeePartShift == kNeeParts, "the tree variants are the upper half of the parts");

using NeeFusedKernel = decltype(&k_nee_fused<MODE_GLOBAL, 0u>);
struct NeeFusedTable { NeeFusedKernel fn[kNeeSceneMask + 1]; };   // by the low four bits; nullptr: no such variant

// the kernels of MODE in this part: one entry for every mask of kNeeVariants that lies in it
template <int MODE, size_t... I>
static NeeFusedTable nee_fused_table(std::index_sequence<I...>) {
	NeeFusedTable t{};
	([&] {
		constexpr uint32_t V = (PTX_NEE_PART >= (int)kNeeParts ? kNeeTreeVariants : kNeeVariants).v[I];
		if constexpr ((V >> kNeePartShift) == PTX_NEE_PART) t.fn[V & kNeeSceneMask] = &k_nee_fused<MODE, V>;
	}(), ...);
	return t;
}

template <int MODE>
static hipError_t launch_nee_fused_mode(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeFusedBuffers& B, size_t lds_bytes,
                                        int grid, hipStream_t stream) {
	static const NeeFusedTable table = nee_fused_table<MODE>(std::make_index_sequence<kNeeVariantCount>{});
	const NeeFusedKernel kernel = table.fn[V & kNeeSceneMask];
	if (!kernel) return hipErrorInvalidValue;
	if (MODE != MODE_GLOBAL) {
		hipError_t e = set_lds(reinterpret_cast<const void*>(kernel), lds_bytes);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(nee_fused_block(V)), MODE != MODE_GLOBAL ? lds_bytes : 0, stream, S, P, Lt, B, S.models, S.surfaces, S.spaces, S.model_space, Ev, ris_m, Pn);
	return hipGetLastError();
}

// Declared for every part, defined by the one compilation of that part: the linker puts the eight together. The definition is an explicit
// specialisation and the template has no body: with one, part 0 naming launch_nee_fused_part<5> would instantiate part 5's kernels itself.
template <uint32_t PART>
hipError_t launch_nee_fused_part(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeFusedBuffers& B, int mode,
                                 size_t lds_bytes, int grid, hipStream_t stream);
template <>
hipError_t launch_nee_fused_part<PTX_NEE_PART>(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeFusedBuffers& B,
                                               int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	if (mode == MODE_LDS) return launch_nee_fused_mode<MODE_LDS>(V, S, P, Lt, Ev, Pn, ris_m, B, lds_bytes, grid, stream);
	if (mode == MODE_HYBRID) return launch_nee_fused_mode<MODE_HYBRID>(V, S, P, Lt, Ev, Pn, ris_m, B, lds_bytes, grid, stream);
	return launch_nee_fused_mode<MODE_GLOBAL>(V, S, P, Lt, Ev, Pn, ris_m, B, lds_bytes, grid, stream);
}

#if PTX_NEE_PART == 0
template <size_t... PART>
static hipError_t launch_nee_fused_in_part(std::index_sequence<PART...>, uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m,
                                           const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	static constexpr decltype(&launch_nee_fused_part<0>) parts[] = {&launch_nee_fused_part<PART>...};
	return parts[V >> kNeePartShift](V, S, P, Lt, Ev, Pn, ris_m, B, mode, lds_bytes, grid, stream);
}

// the variant: nee_select_variant (nee_core.hpp), as for launch_nee_shade
hipError_t launch_nee_fused(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeFusedBuffers& B,
                            int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	uint32_t V, ris_m;
	const hipError_t e = nee_select_variant(S, Lt, Ev, Pn, sampler_pdf, candidates, V, ris_m);
	if (e != hipSuccess) return e;
	return launch_nee_fused_in_part(std::make_index_sequence<kNeeFusedParts>{}, V, S, P, Lt, Ev, Pn, ris_m, B, mode, lds_bytes, grid, stream);
}
#endif

}  // namespace ptx
