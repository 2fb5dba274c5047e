// Next-event estimation towards emissive triangles (ptx_render_nee): the LIB estimator of shade_vertex<SUN, ALPHA, TEX, false> plus one
// light sample per continuing vertex, combined with the BSDF-sampled emission by the balance heuristic (include/ptx.h has the estimator).
// A classic wavefront in the shape of aov.hip: the closest hits of the live rays and of the shadow rays come from the scene's own
// intersect route (launch_intersect / launch_wf_intersect, issued by ptx_api.cpp between the kernels of this file).
//   k_nee_generate   sample id -> camera ray; path state (T = 1, depth 0) and the sample's radiance record (0, 0, 0, 1)
//   k_nee_shade      one path vertex per lane: LIB's rules in LIB's order, the emission weighted, the light sample taken before the BSDF
//                    sample. Shadow rays (sun or shadow catcher, and light) are appended densely to the round's shadow stream, the
//                    continuation to the next round's path stream (wave ballot + lane prefix count, one atomic per wave and stream)
//   k_nee_settle     one lane per path of the round: adds the sun term if unoccluded, then the light term if the shadow ray's closest hit
//                    is the sampled triangle (an environment sample's: if it hit nothing); appends the pass-through ray of a lit shadow catcher
// A sample's radiance lives in a record by sample id: vertex k's emission is added by round k's shade kernel, its sun and light terms by
// round k's settle kernel, vertex k + 1's by the next round — a fixed order without float atomics. The pass ends with k_resolve.
// Numerics as in kernels.hip: IEEE binary32 in the written order, no contraction.
#include "nee_core.hpp"

namespace ptx {

constexpr int kNeeBlock = 256;

// This file is compiled four times, with -DPTX_NEE_PART=0 .. 3, so that the quarters of k_nee_shade's variants build side by side. Here a part
// is the PUN and LTREE bits of the mask (nee_core.hpp), 48 kernels each: part 0 is everything without either, part 1 the PUN variants, parts
// 2 and 3 the tree variants (kNeeTreeVariants) without and with PUN; parts 1 to 3 hold launch_nee_shade_part<part> alone.
#ifndef PTX_NEE_PART
#error "nee.hip is compiled once per quarter of the variants: -DPTX_NEE_PART=<0..3> (the Makefile's NEE_SHADE_PARTS)"
#endif
static_assert(PTX_NEE_PART >= 0 && PTX_NEE_PART <= 3, "a part of this file is the PUN and LTREE bits of a variant");
constexpr uint32_t kNeeShadePartShift = 6, kNeeShadePartMask = (1u << kNeeShadePartShift) - 1;
static_assert(NEE_PUN == 1u << kNeeShadePartShift && NEE_LTREE == 2u << kNeeShadePartShift, "the four parts are split by PUN and LTREE");

#if PTX_NEE_PART == 0
__global__ void __launch_bounds__(kNeeBlock) k_nee_generate(DevScene S0, RenderParams P, NeeStream out, float4* __restrict__ L, uint32_t n, RenderMotion Mo) {
	const uint32_t i = blockIdx.x * kNeeBlock + threadIdx.x;
	if (i >= n) return;
	uint32_t px, py, sample;
	nee_sample_of(P, i, px, py, sample);
	DevScene S = S0;
	if (Mo.camera_moved) camera_at(S, Mo, sample_time(P, Mo, py * P.W + px, sample));   // the camera of the sample's own time (wave-uniform test)
	V3 o, d;
	camera_ray(S, P, px, py, sample, o, d);
	out.ox[i] = o.x; out.oy[i] = o.y; out.oz[i] = o.z;
	out.dx[i] = d.x; out.dy[i] = d.y; out.dz[i] = d.z;
	out.tx[i] = 1.0f; out.ty[i] = 1.0f; out.tz[i] = 1.0f; out.pp[i] = 0.0f;
	out.id[i] = i; out.dp[i] = 0u;
	L[i] = make_float4(0.f, 0.f, 0.f, 1.0f);
}
#endif

// dense append: one atomic per wave reserves the wave's entries, the lane prefix count places them. `second` entries follow the wave's
// `first` entries. Returns the lane's positions (valid where its flag is set).
DEV void nee_append2(bool first, bool second, uint32_t* counter, uint32_t& pos_first, uint32_t& pos_second) {
	const uint64_t m1 = __ballot(first), m2 = __ballot(second);
	pos_first = pos_second = 0;
	if ((m1 | m2) == 0) return;
	const uint32_t n1 = (uint32_t)__popcll(m1);
	const int leader = __ffsll((long long)(m1 | m2)) - 1;
	uint32_t base = 0;
	if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(counter, n1 + (uint32_t)__popcll(m2));
	base = __shfl(base, leader);
	pos_first = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
	pos_second = base + n1 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0u));
}

// One vertex of every live path: loads the hit and the path state of entry i, runs nee_vertex (nee_core.hpp) and stores what it returns.
// V: the variant (nee_core.hpp has the bits). Ev is read by the ENV variants alone, ris_m by the RIS variants, Pn by the PUN variants; the
// LTREE variants alone read and write the streams' x_prev arrays (Xi beside `in`, Xo beside `out`).
template <uint32_t V>
__global__ void __launch_bounds__(kNeeBlock) k_nee_shade(DevScene S, RenderParams P, NeeLights Lt, NeeStream in, NeeHits H, uint32_t n, NeeStream out, NeeShadow W,
                                                         uint32_t* __restrict__ cnt, float4* __restrict__ Lrec, NeeEnv Ev, uint32_t ris_m, NeePunctual Pn, RenderMotion Mo, NeePrev Xi, NeePrev Xo) {
	const uint32_t i = blockIdx.x * kNeeBlock + threadIdx.x;
	NeeVertex v;
	float u = 0;   // the path's time; computed under active motion alone
	V3 o = {0, 0, 0}, d = {0, 0, 1}, T = {1, 1, 1};
	float p_prev = 0;
	uint32_t id = 0, depth = 0, pass = 0;
	constexpr bool LTREE = (V & NEE_LTREE) != 0;
	V3 x_prev = {0, 0, 0};
	if (i < n) {
		id = in.id[i];
		const uint32_t dp = in.dp[i];
		depth = dp >> 16; pass = dp & 0xFFFFu;
		d = mk(in.dx[i], in.dy[i], in.dz[i]);
		T = mk(in.tx[i], in.ty[i], in.tz[i]);
		p_prev = in.pp[i];
		if constexpr (LTREE)
			if (depth != 0) x_prev = mk(Xi.px[i], Xi.py[i], Xi.pz[i]);   // set by the vertex that drew the BSDF sample; none has at depth 0
		uint32_t px, py, sample;
		nee_sample_of(P, id, px, py, sample);
		const uint32_t pixel = py * P.W + px;
		const float4 l4 = Lrec[id];
		V3 L = mk(l4.x, l4.y, l4.z);
		const int32_t surf = H.surface[i];
		bool moved = false;
		XformRecs Xm;
		if (Mo.active) {   // wave-uniform: a kernel argument
			u = sample_time(P, Mo, pixel, sample);
			if (Mo.models_moved && surf >= 0) {
				const uint32_t m = S.surfaces[surf].model;
				moved = Mo.models.moved[m] != 0u;
				if (moved) model_records_at(Mo.models, m, u, Xm);   // the hit surface's records at the path's time
			}
		}
		if (nee_vertex<V>(S, P, Lt, Ev, ris_m, pixel, sample, surf, (uint32_t)H.triangle[i], H.b1[i], H.b2[i], H.distance[i], o, d, T, L, p_prev, depth, pass, v, Pn, moved, Xm, LTREE ? &x_prev : nullptr))
			Lrec[id] = make_float4(L.x, L.y, L.z, l4.w);
	}
	// shadow rays of the round: at most two per path, so every position is below twice the round's paths
	uint32_t sp, lp;
	nee_append2(v.want_sun, v.want_light, cnt + 1, sp, lp);
	if (v.want_sun) {
		W.ox[sp] = v.sun_o.x; W.oy[sp] = v.sun_o.y; W.oz[sp] = v.sun_o.z;
		W.dx[sp] = v.sun_d.x; W.dy[sp] = v.sun_d.y; W.dz[sp] = v.sun_d.z;
		W.sx[i] = v.sun_x.x; W.sy[i] = v.sun_x.y; W.sz[i] = v.sun_x.z;
		if (Mo.active) W.tm[sp] = u;   // every ray of the sample's path carries its time
	}
	if (v.want_light) {
		W.ox[lp] = v.lo.x; W.oy[lp] = v.lo.y; W.oz[lp] = v.lo.z;
		W.dx[lp] = v.ld.x; W.dy[lp] = v.ld.y; W.dz[lp] = v.ld.z;
		W.lx[i] = v.lx.x; W.ly[i] = v.lx.y; W.lz[i] = v.lx.z;
		W.exp_surf[i] = v.exp_surf; W.exp_tri[i] = v.exp_tri;
		if (Mo.active) W.tm[lp] = u;
	}
	if (i < n) {
		W.sun_pos[i] = v.want_sun ? (sp | (v.catcher_req ? kNeeCatcher : 0u)) : kNeeNone;
		W.light_pos[i] = v.want_light ? lp : kNeeNone;
	}
	const uint64_t lm = __ballot(v.want_light);
	if (lm != 0 && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)lm) - 1)) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + 2), (unsigned long long)__popcll(lm));
	// the continuation: a lane appends at most one entry, and a pending shadow catcher none here, so every position is below n
	uint32_t pos, unused;
	nee_append2(v.alive, false, cnt, pos, unused);
	if (v.alive) {
		out.ox[pos] = o.x; out.oy[pos] = o.y; out.oz[pos] = o.z;
		out.dx[pos] = d.x; out.dy[pos] = d.y; out.dz[pos] = d.z;
		out.tx[pos] = T.x; out.ty[pos] = T.y; out.tz[pos] = T.z; out.pp[pos] = p_prev;
		out.id[pos] = id; out.dp[pos] = (depth << 16) | pass;
		if constexpr (LTREE) { Xo.px[pos] = x_prev.x; Xo.py[pos] = x_prev.y; Xo.pz[pos] = x_prev.z; }
	}
}

#if PTX_NEE_PART == 0
// The answers of the round's shadow rays (SH: their closest hits). One lane per path of the round, sun before light.
// PUN: the round may hold punctual samples' rays (kNeePunctualRay): visible iff nothing is hit nearer than the light.
// LTREE: the streams carry x_prev (Xi, Xo), and a lit catcher's pass-through writes its entry of Xo.
template <bool PUN, bool LTREE>
__global__ void __launch_bounds__(kNeeBlock) k_nee_settle(NeeStream in, uint32_t n, NeeShadow W, NeeHits SH, NeeStream out, uint32_t* __restrict__ cnt, float4* __restrict__ Lrec, NeePrev Xi, NeePrev Xo) {
	const uint32_t i = blockIdx.x * kNeeBlock + threadIdx.x;
	bool through = false, visible = false;
	if (i < n) {
		const uint32_t sw = W.sun_pos[i], lp = W.light_pos[i];
		if (sw != kNeeNone || lp != kNeeNone) {
			const uint32_t id = in.id[i];
			float4 v = Lrec[id];
			bool store = false;
			if (sw != kNeeNone) {
				const bool occluded = SH.surface[sw & ~kNeeCatcher] >= 0;
				if (sw & kNeeCatcher) through = !occluded && ((in.dp[i] & 0xFFFFu) + 1u) <= 4096u;   // shadowed: the path ends with what it has
				else if (!occluded) { v.x += W.sx[i]; v.y += W.sy[i]; v.z += W.sz[i]; store = true; }
			}
			if (lp != kNeeNone) {
				const uint32_t es = W.exp_surf[i];
				if (PUN && es == kNeePunctualRay) visible = SH.surface[lp] < 0 || !(SH.distance[lp] < __uint_as_float(W.exp_tri[i]));
				else visible = es == kNeeEnvRay ? SH.surface[lp] < 0 : (SH.surface[lp] == (int32_t)es && SH.triangle[lp] == (int32_t)W.exp_tri[i]);
				if (visible) { v.x += W.lx[i]; v.y += W.ly[i]; v.z += W.lz[i]; store = true; }
			}
			if (store) Lrec[id] = v;
		}
	}
	const uint64_t vm = __ballot(visible);
	if (vm != 0 && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)vm) - 1)) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + 4), (unsigned long long)__popcll(vm));
	// lit catcher = fully transparent: same depth, next pass. Such a path appended nothing in k_nee_shade, so the round's appends stay below n
	uint32_t pos, unused;
	nee_append2(through, false, cnt, pos, unused);
	if (through) {
		const V3 dn = normalize(mk(in.dx[i], in.dy[i], in.dz[i]));
		out.ox[pos] = W.sx[i]; out.oy[pos] = W.sy[i]; out.oz[pos] = W.sz[i];
		out.dx[pos] = dn.x; out.dy[pos] = dn.y; out.dz[pos] = dn.z;
		out.tx[pos] = in.tx[i]; out.ty[pos] = in.ty[i]; out.tz[pos] = in.tz[i]; out.pp[pos] = in.pp[i];
		out.id[pos] = in.id[i]; out.dp[pos] = in.dp[i] + 1u;
		// a catcher is a depth-0 vertex, where no vertex has set x_prev yet and k_nee_shade does not read it: the entry's x_prev is 0
		if constexpr (LTREE) { Xo.px[pos] = 0.0f; Xo.py[pos] = 0.0f; Xo.pz[pos] = 0.0f; }
	}
}

#endif

// ------------------------------------------------------------------------------------ launchers
#if PTX_NEE_PART == 0
hipError_t launch_nee_generate(const DevScene& S, const RenderParams& P, const NeeStream& out, float4* L, uint32_t n, const RenderMotion& Mo, hipStream_t stream) {
	hipLaunchKernelGGL(k_nee_generate, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, S, P, out, L, n, Mo);
	return hipGetLastError();
}
#endif

using NeeShadeKernel = decltype(&k_nee_shade<0u>);
struct NeeShadeTable { NeeShadeKernel fn[kNeeShadePartMask + 1]; };   // by the bits below PUN; nullptr: no such variant

// the kernels of this part: one entry for every mask of kNeeVariants that lies in it
template <size_t... I>
static NeeShadeTable nee_shade_table(std::index_sequence<I...>) {
	NeeShadeTable t{};
	([&] {
		constexpr uint32_t V = (PTX_NEE_PART >= 2 ? kNeeTreeVariants : kNeeVariants).v[I];
		if constexpr ((V >> kNeeShadePartShift) == PTX_NEE_PART) t.fn[V & kNeeShadePartMask] = &k_nee_shade<V>;
	}(), ...);
	return t;
}

// Declared for both parts, defined by the one compilation of that part, as an explicit specialisation of a template without a body
// (nee_fused.hip has the reason): the linker puts the two together.
template <uint32_t PART>
hipError_t launch_nee_shade_part(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeStream& in, const NeeHits& H,
                                 uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, const RenderMotion& Mo, const NeePrev& Xi, const NeePrev& Xo, hipStream_t stream);
template <>
hipError_t launch_nee_shade_part<PTX_NEE_PART>(uint32_t V, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeStream& in,
                                               const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, const RenderMotion& Mo, const NeePrev& Xi, const NeePrev& Xo,
                                               hipStream_t stream) {
	static const NeeShadeTable table = nee_shade_table(std::make_index_sequence<kNeeVariantCount>{});
	const NeeShadeKernel kernel = table.fn[V & kNeeShadePartMask];
	if (!kernel) return hipErrorInvalidValue;
	hipLaunchKernelGGL(kernel, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, S, P, Lt, in, H, n, out, W, cnt, L, Ev, ris_m, Pn, Mo, Xi, Xo);
	return hipGetLastError();
}

#if PTX_NEE_PART == 0
// the variant: nee_select_variant (nee_core.hpp), as for launch_nee_fused
hipError_t launch_nee_shade(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeStream& in,
                            const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, const RenderMotion& Mo, const NeePrev& Xi, const NeePrev& Xo,
                            hipStream_t stream) {
	uint32_t V, ris_m;
	const hipError_t e = nee_select_variant(S, Lt, Ev, Pn, sampler_pdf, candidates, V, ris_m);
	if (e != hipSuccess) return e;
	static constexpr decltype(&launch_nee_shade_part<0>) parts[] = {&launch_nee_shade_part<0>, &launch_nee_shade_part<1>, &launch_nee_shade_part<2>, &launch_nee_shade_part<3>};
	const auto part = parts[V >> kNeeShadePartShift];
	return part(V, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L, Mo, Xi, Xo, stream);
}

hipError_t launch_nee_settle(const NeeStream& in, uint32_t n, const NeeShadow& W, const NeeHits& SH, const NeeStream& out, uint32_t* cnt, float4* L, bool punctual, const NeePrev& Xi, const NeePrev& Xo, hipStream_t stream) {
	const dim3 grid((n + kNeeBlock - 1) / kNeeBlock), block(kNeeBlock);
	const bool tree = Xi.px != nullptr;
	if (tree && punctual) hipLaunchKernelGGL((k_nee_settle<true, true>), grid, block, 0, stream, in, n, W, SH, out, cnt, L, Xi, Xo);
	else if (tree) hipLaunchKernelGGL((k_nee_settle<false, true>), grid, block, 0, stream, in, n, W, SH, out, cnt, L, Xi, Xo);
	else if (punctual) hipLaunchKernelGGL((k_nee_settle<true, false>), grid, block, 0, stream, in, n, W, SH, out, cnt, L, Xi, Xo);
	else hipLaunchKernelGGL((k_nee_settle<false, false>), grid, block, 0, stream, in, n, W, SH, out, cnt, L, Xi, Xo);
	return hipGetLastError();
}
#endif

}  // namespace ptx
