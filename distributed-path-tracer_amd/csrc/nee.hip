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

// This file is compiled twice, so that the two halves of k_nee_shade's variants build side by side: as itself (everything but the PUN
// variants) and through nee_punctual.hip, which defines PTX_NEE_PUNCTUAL_TU (the PUN variants and launch_nee_shade_punctual alone).
#ifndef PTX_NEE_PUNCTUAL_TU
__global__ void __launch_bounds__(kNeeBlock) k_nee_generate(DevScene S, RenderParams P, NeeStream out, float4* __restrict__ L, uint32_t n) {
	const uint32_t i = blockIdx.x * kNeeBlock + threadIdx.x;
	if (i >= n) return;
	uint32_t px, py, sample;
	nee_sample_of(P, i, px, py, sample);
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
// TEX / ALPHA / SUN compile the texture lookups / the pass-through and catcher code / the sun request in, as the render variants do;
// ENV the environment sample and the miss weight (PTX_NEE_ENV_SAMPLES; TEX only: a map implies the TEX variants). Ev, the last argument, is
// read by the ENV variants alone. SPDF: the weights of PTX_NEE_SAMPLER_PDF. RIS: the light sample chosen among ris_m candidates
// (PTX_NEE_CANDIDATES); the other variants do not read ris_m. PUN: punctual lights on the scene (Pn), a third kind of candidate; the other
// variants do not read Pn.
template <bool TEX, bool ALPHA, bool SUN, bool ENV, bool SPDF = false, bool RIS = false, bool PUN = false>
__global__ void __launch_bounds__(kNeeBlock) k_nee_shade(DevScene S, RenderParams P, NeeLights Lt, NeeStream in, NeeHits H, uint32_t n, NeeStream out, NeeShadow W,
                                                         uint32_t* __restrict__ cnt, float4* __restrict__ Lrec, NeeEnv Ev, uint32_t ris_m, NeePunctual Pn) {
	const uint32_t i = blockIdx.x * kNeeBlock + threadIdx.x;
	NeeVertex v;
	V3 o = {0, 0, 0}, d = {0, 0, 1}, T = {1, 1, 1};
	float p_prev = 0;
	uint32_t id = 0, depth = 0, pass = 0;
	if (i < n) {
		id = in.id[i];
		const uint32_t dp = in.dp[i];
		depth = dp >> 16; pass = dp & 0xFFFFu;
		d = mk(in.dx[i], in.dy[i], in.dz[i]);
		T = mk(in.tx[i], in.ty[i], in.tz[i]);
		p_prev = in.pp[i];
		uint32_t px, py, sample;
		nee_sample_of(P, id, px, py, sample);
		const uint32_t pixel = py * P.W + px;
		const float4 l4 = Lrec[id];
		V3 L = mk(l4.x, l4.y, l4.z);
		if (nee_vertex<TEX, ALPHA, SUN, ENV, SPDF, RIS, PUN>(S, P, Lt, Ev, ris_m, pixel, sample, H.surface[i], (uint32_t)H.triangle[i], H.b1[i], H.b2[i], H.distance[i], o, d, T, L, p_prev, depth, pass, v, Pn))
			Lrec[id] = make_float4(L.x, L.y, L.z, l4.w);
	}
	// shadow rays of the round: at most two per path, so every position is below twice the round's paths
	uint32_t sp, lp;
	nee_append2(v.want_sun, v.want_light, cnt + 1, sp, lp);
	if (v.want_sun) {
		W.ox[sp] = v.sun_o.x; W.oy[sp] = v.sun_o.y; W.oz[sp] = v.sun_o.z;
		W.dx[sp] = v.sun_d.x; W.dy[sp] = v.sun_d.y; W.dz[sp] = v.sun_d.z;
		W.sx[i] = v.sun_x.x; W.sy[i] = v.sun_x.y; W.sz[i] = v.sun_x.z;
	}
	if (v.want_light) {
		W.ox[lp] = v.lo.x; W.oy[lp] = v.lo.y; W.oz[lp] = v.lo.z;
		W.dx[lp] = v.ld.x; W.dy[lp] = v.ld.y; W.dz[lp] = v.ld.z;
		W.lx[i] = v.lx.x; W.ly[i] = v.lx.y; W.lz[i] = v.lx.z;
		W.exp_surf[i] = v.exp_surf; W.exp_tri[i] = v.exp_tri;
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
	}
}

#ifndef PTX_NEE_PUNCTUAL_TU
// The answers of the round's shadow rays (SH: their closest hits). One lane per path of the round, sun before light.
// PUN: the round may hold punctual samples' rays (kNeePunctualRay): visible iff nothing is hit nearer than the light.
template <bool PUN>
__global__ void __launch_bounds__(kNeeBlock) k_nee_settle(NeeStream in, uint32_t n, NeeShadow W, NeeHits SH, NeeStream out, uint32_t* __restrict__ cnt, float4* __restrict__ Lrec) {
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
	}
}

#endif

// ------------------------------------------------------------------------------------ launchers
#ifndef PTX_NEE_PUNCTUAL_TU
hipError_t launch_nee_generate(const DevScene& S, const RenderParams& P, const NeeStream& out, float4* L, uint32_t n, hipStream_t stream) {
	hipLaunchKernelGGL(k_nee_generate, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, S, P, out, L, n);
	return hipGetLastError();
}
#endif

template <bool TEX, bool ALPHA, bool ENV, bool SPDF, bool RIS, bool PUN>
static void nee_shade_sun(bool sun, dim3 grid, hipStream_t stream, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeStream& in,
                          const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L) {
	if (sun) hipLaunchKernelGGL((k_nee_shade<TEX, ALPHA, true, ENV, SPDF, RIS, PUN>), grid, dim3(kNeeBlock), 0, stream, S, P, Lt, in, H, n, out, W, cnt, L, Ev, ris_m, Pn);
	else hipLaunchKernelGGL((k_nee_shade<TEX, ALPHA, false, ENV, SPDF, RIS, PUN>), grid, dim3(kNeeBlock), 0, stream, S, P, Lt, in, H, n, out, W, cnt, L, Ev, ris_m, Pn);
}

template <bool SPDF, bool RIS, bool PUN>
static hipError_t launch_nee_shade_variant(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, uint32_t ris_m, const NeeStream& in, const NeeHits& H, uint32_t n,
                                        const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, hipStream_t stream) {
	const dim3 grid((n + kNeeBlock - 1) / kNeeBlock);
	const bool sun = S.sun.present != 0;
	if (Ev.row_cdf) {   // a table means a map, and a map means the TEX variants
		if (!S.any_texture || S.env_tex < 0) return hipErrorInvalidValue;
		if (S.any_alpha) nee_shade_sun<true, true, true, SPDF, RIS, PUN>(sun, grid, stream, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L);
		else nee_shade_sun<true, false, true, SPDF, RIS, PUN>(sun, grid, stream, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L);
	} else if (S.any_texture) {
		if (S.any_alpha) nee_shade_sun<true, true, false, SPDF, RIS, PUN>(sun, grid, stream, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L);
		else nee_shade_sun<true, false, false, SPDF, RIS, PUN>(sun, grid, stream, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L);
	} else {
		if (S.any_alpha) nee_shade_sun<false, true, false, SPDF, RIS, PUN>(sun, grid, stream, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L);
		else nee_shade_sun<false, false, false, SPDF, RIS, PUN>(sun, grid, stream, S, P, Lt, Ev, Pn, ris_m, in, H, n, out, W, cnt, L);
	}
	return hipGetLastError();
}

// the four quarters (SPDF x RIS) of one half (PUN) of the variants
template <bool PUN>
static hipError_t launch_nee_shade_half(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeStream& in,
                                        const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, hipStream_t stream) {
	if (candidates > 1)
		return sampler_pdf ? launch_nee_shade_variant<true, true, PUN>(S, P, Lt, Ev, Pn, candidates, in, H, n, out, W, cnt, L, stream)
		                   : launch_nee_shade_variant<false, true, PUN>(S, P, Lt, Ev, Pn, candidates, in, H, n, out, W, cnt, L, stream);
	return sampler_pdf ? launch_nee_shade_variant<true, false, PUN>(S, P, Lt, Ev, Pn, 1u, in, H, n, out, W, cnt, L, stream)
	                   : launch_nee_shade_variant<false, false, PUN>(S, P, Lt, Ev, Pn, 1u, in, H, n, out, W, cnt, L, stream);
}

hipError_t launch_nee_shade_punctual(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeStream& in,
                                     const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, hipStream_t stream);
#ifdef PTX_NEE_PUNCTUAL_TU
hipError_t launch_nee_shade_punctual(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeStream& in,
                                     const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, hipStream_t stream) {
	return launch_nee_shade_half<true>(S, P, Lt, Ev, Pn, sampler_pdf, candidates, in, H, n, out, W, cnt, L, stream);
}
#else
// sampler_pdf: the variants of PTX_NEE_SAMPLER_PDF; candidates > 1: the RIS variants with M = candidates (PTX_NEE_CANDIDATES); Pn.n != 0: the PUN variants
hipError_t launch_nee_shade(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeStream& in,
                            const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, hipStream_t stream) {
	if (Pn.n != 0) return launch_nee_shade_punctual(S, P, Lt, Ev, Pn, sampler_pdf, candidates, in, H, n, out, W, cnt, L, stream);
	return launch_nee_shade_half<false>(S, P, Lt, Ev, Pn, sampler_pdf, candidates, in, H, n, out, W, cnt, L, stream);
}

hipError_t launch_nee_settle(const NeeStream& in, uint32_t n, const NeeShadow& W, const NeeHits& SH, const NeeStream& out, uint32_t* cnt, float4* L, bool punctual, hipStream_t stream) {
	if (punctual) hipLaunchKernelGGL(k_nee_settle<true>, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, in, n, W, SH, out, cnt, L);
	else hipLaunchKernelGGL(k_nee_settle<false>, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, in, n, W, SH, out, cnt, L);
	return hipGetLastError();
}
#endif

}  // namespace ptx
