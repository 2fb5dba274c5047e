// Next-event estimation towards emissive triangles (ptx_render_nee): the LIB estimator of shade_vertex<SUN, ALPHA, TEX, false> plus one
// light sample per continuing vertex, combined with the BSDF-sampled emission by the balance heuristic (include/ptx.h has the estimator).
// A classic wavefront in the shape of aov.hip: the closest hits of the live rays and of the shadow rays come from the scene's own
// intersect route (launch_intersect / launch_wf_intersect, issued by ptx_api.cpp between the kernels of this file).
//   k_nee_generate   sample id -> camera ray; path state (T = 1, depth 0) and the sample's radiance record (0, 0, 0, 1)
//   k_nee_shade      one path vertex per lane: LIB's rules in LIB's order, the emission weighted, the light sample taken before the BSDF
//                    sample. Shadow rays (sun or shadow catcher, and light) are appended densely to the round's shadow stream, the
//                    continuation to the next round's path stream (wave ballot + lane prefix count, one atomic per wave and stream)
//   k_nee_settle     one lane per path of the round: adds the sun term if unoccluded, then the light term if the shadow ray's closest hit
//                    is the sampled triangle; appends the pass-through ray of a lit shadow catcher
// A sample's radiance lives in a record by sample id: vertex k's emission is added by round k's shade kernel, its sun and light terms by
// round k's settle kernel, vertex k + 1's by the next round — a fixed order without float atomics. The pass ends with k_resolve.
// Numerics as in kernels.hip: IEEE binary32 in the written order, no contraction.
#include "device_core.hpp"

namespace ptx {

constexpr int kNeeBlock = 256;
enum { BLOCK_LIGHT = 3 };   // Philox block of the light sample's draws (BLOCK_SURFACE / BLOCK_SUN / BLOCK_JITTER: device_core.hpp)

// sample id within the pass (sample-major, pixel-minor) -> image pixel and global sample index, as k_render_pass enumerates them
DEV void nee_sample_of(const RenderParams& P, uint32_t id, uint32_t& px, uint32_t& py, uint32_t& sample) {
	const uint32_t s_local = id / P.n_pixels;
	uint32_t p_local = id - s_local * P.n_pixels;
	if (P.pixels) p_local = P.pixels[p_local];
	px = P.x0 + p_local % P.w; py = P.y0 + p_local / P.w;
	sample = P.sample0 + s_local;
}

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

// entry of (surface, local triangle) in the light list, or -1: the list is ordered by surface, then by triangle
DEV int nee_find_light(const NeeLights& Lt, uint32_t surface, uint32_t tri) {
	const int first = Lt.surf_first[surface];
	if (first < 0) return -1;
	uint32_t lo = (uint32_t)first, hi = Lt.n;   // the entry, if any, is in [lo, hi)
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		const uint2 e = Lt.tris[mid];
		if (e.x < surface || (e.x == surface && e.y < tri)) lo = mid + 1; else hi = mid;
	}
	if (lo >= Lt.n) return -1;
	const uint2 e = Lt.tris[lo];
	return (e.x == surface && e.y == tri) ? (int)lo : -1;
}

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

// One vertex of every live path. TEX / ALPHA / SUN compile the texture lookups / the pass-through and catcher code / the sun request in,
// as the render variants do. The statements between the marks are shade_vertex<SUN, ALPHA, TEX, false>'s, in its order.
template <bool TEX, bool ALPHA, bool SUN>
__global__ void __launch_bounds__(kNeeBlock) k_nee_shade(DevScene S, RenderParams P, NeeLights Lt, NeeStream in, NeeHits H, uint32_t n, NeeStream out, NeeShadow W,
                                                         uint32_t* __restrict__ cnt, float4* __restrict__ Lrec) {
	const uint32_t i = blockIdx.x * kNeeBlock + threadIdx.x;
	bool alive = false, want_sun = false, want_light = false, catcher_req = false;
	V3 o = {0, 0, 0}, d = {0, 0, 1}, T = {1, 1, 1};
	V3 sun_o = o, sun_d = d, sun_x = o, lo = o, ld = d, lx = o;
	float p_prev = 0;
	uint32_t id = 0, depth = 0, pass = 0, exp_surf = 0, exp_tri = 0;
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
		const int32_t surf = H.surface[i];
		const float4 l4 = Lrec[id];
		V3 L = mk(l4.x, l4.y, l4.z);
		bool store = false;
		do {
			if (surf < 0) {   // miss: environment
				V3 env = mk(P.env[0], P.env[1], P.env[2]);
				if constexpr (TEX) {
					if (S.env_tex >= 0) {
						const float4 e = tex_sample(S, S.env_tex, atan2f(d.z, d.x) * 0.1591F + 0.5F, asinf(d.y) * 0.3183F + 0.5F);
						env = mk(e.x, e.y, e.z) * env;
					}
				}
				L = L + T * env;
				store = true;
				break;
			}
			const uint32_t tri = (uint32_t)H.triangle[i];
			const ShadeRec& R = S.shade[surf];
			Surf sf;
			hit_attributes(S, R, tri + S.surfaces[surf].tri_base, H.b1[i], H.b2[i], sf);
			const MaterialRec& mt = R.mat;
			const MatEval me = material_eval<TEX>(S, mt, sf.u, sf.v);
			float roughness = me.roughness;
			const bool last = depth + 1 == P.bounces;
			float4 rnd = make_float4(0, 0, 0, 0);
			if (ALPHA || !last) rnd = draws(P, pixel, sample, depth, pass, BLOCK_SURFACE);
			if constexpr (ALPHA) {
				const bool transparent = !(me.opacity == 1.0f || fabsf(me.opacity - 1.0f) < kEps) && rnd.x > me.opacity;
				if (transparent) {
					o = sf.pos + d * kEps;
					d = normalize(d);
					pass++;
					alive = pass <= 4096;
					break;
				}
			}
			const V3 normal = shading_normal(sf, me.normal_ts), outcoming = -d;
			if (dot(normal, outcoming) <= 0) break;
			roughness = pmax(roughness, 0.05F);
			float spec_prob = 0;
			if (!last || (SUN && S.sun.present)) {
				spec_prob = fresnel_schlick(outcoming, reflect3(-outcoming, normal), mt.ior);
				spec_prob = pmax(spec_prob, me.metallic);
			}
			if constexpr (SUN) {
				const bool catcher = ALPHA && mt.shadow_catcher && depth == 0;
				bool sampled = false;
				V3 din = mk(0, 0, 0);
				if (S.sun.present) {
					const float4 sr = draws(P, pixel, sample, depth, pass, BLOCK_SUN);
					V3 c = mulmv(S.sun.basis, mk(0, 0, 1));
					c = rand_cone_vec(sr.x, cosf(sr.y * S.sun.angular_radius), c);
					const V3 cn = normalize(c);
					din = c;
					sampled = dot(normal, c) > 0;
					if (sampled) { sun_o = sf.pos + c * kEps; sun_d = cn; }
				}
				if (sampled) {
					want_sun = true;
					if (catcher) {   // the answer decides between the pass-through and the end of the path (k_nee_settle)
						catcher_req = true;
						sun_x = sf.pos + d * kEps;
						break;
					}
					float pdf_unused;
					const V3 brdf = eval_brdf(normal, outcoming, din, me.albedo, roughness, me.metallic, spec_prob, pdf_unused);
					const V3 e = mk(S.sun.energy[0], S.sun.energy[1], S.sun.energy[2]);
					const float pdf = lerpf(1.0f, 1.0f, spec_prob);
					const V3 v = brdf * e / pmax(pdf, kEps);
					const V3 direct_out = mk(clampf(v.x, 0, e.x), clampf(v.y, 0, e.y), clampf(v.z, 0, e.z));
					sun_x = T * direct_out;
				}
			}
			// ---- emission, weighted against the light sample that could have produced this path
			V3 em = T * me.emissive10;
			if (Lt.n != 0 && depth != 0 && pass == 0) {
				const int k = nee_find_light(Lt, (uint32_t)surf, tri);
				if (k >= 0) {
					const float4 g = Lt.geom[k];
					const float cg = fabsf(dot(mk(g.x, g.y, g.z), d));
					const float dist = H.distance[i];
					const float p_l = (dist * dist) / (cg * Lt.area);
					em = em * (p_prev / (p_prev + p_l));
				}
			}
			L = L + em;
			store = true;
			if (last) break;
			// ---- light sample
			if (Lt.n != 0) {
				const float4 r = draws(P, pixel, sample, depth, pass, BLOCK_LIGHT);
				uint32_t a = 0, b = Lt.n;   // first entry with r.x < cdf
				while (a < b) {
					const uint32_t mid = a + (b - a) / 2;
					if (r.x < Lt.cdf[mid]) b = mid; else a = mid + 1;
				}
				const uint32_t k = a < Lt.n - 1 ? a : Lt.n - 1;
				const float su = sqrt_exact(r.y), beta = su * (1 - r.z), gamma = su * r.z;
				const uint2 lt = Lt.tris[k];
				const ShadeRec& Ry = S.shade[lt.x];
				Surf sy;
				hit_attributes(S, Ry, lt.y + S.surfaces[lt.x].tri_base, beta, gamma, sy);
				const MatEval my = material_eval<TEX>(S, Ry.mat, sy.u, sy.v);
				const V3 n_y = shading_normal(sy, my.normal_ts), Le = my.emissive10;
				const V3 v = sy.pos - sf.pos;
				const float dist2 = dot(v, v);
				if (dist2 > 0) {
					const V3 w = v / sqrt_exact(dist2);
					const float4 g = Lt.geom[k];
					const float cg = fabsf(dot(mk(g.x, g.y, g.z), w));
					if (dot(normal, w) > 0 && dot(n_y, -w) > 0 && cg > 0 && pmax(Le.x, pmax(Le.y, Le.z)) > 0) {
						float pdf;
						const V3 brdf = eval_brdf(normal, outcoming, w, me.albedo, roughness, me.metallic, spec_prob, pdf);
						const float pe = pmax(pdf, kEps);
						const V3 q = brdf / pe;
						const V3 qc = mk(clampf(q.x, 0, 1), clampf(q.y, 0, 1), clampf(q.z, 0, 1));
						const float p_l = dist2 / (cg * Lt.area);
						const float wl = pe / (pe + p_l);
						lx = ((T * qc) * wl) * Le;
						lo = sf.pos + w * kEps;
						ld = w;
						exp_surf = lt.x; exp_tri = lt.y;
						want_light = true;
					}
				}
			}
			// ---- BSDF sample
			const V3 inc = importance_sample(rnd.y < spec_prob, rnd.z, rnd.w, normal, outcoming, roughness);
			if (!(dot(normal, inc) > 0)) break;
			float pdf;
			const V3 brdf = eval_brdf(normal, outcoming, inc, me.albedo, roughness, me.metallic, spec_prob, pdf);
			const float pe = pmax(pdf, kEps);
			const V3 q = brdf / pe;
			T = T * mk(clampf(q.x, 0, 1), clampf(q.y, 0, 1), clampf(q.z, 0, 1));
			p_prev = pe;
			o = sf.pos + inc * kEps;
			d = normalize(inc);
			depth++;
			pass = 0;
			alive = depth != P.bounces;
		} while (false);
		if (store) Lrec[id] = make_float4(L.x, L.y, L.z, l4.w);
	}
	// shadow rays of the round: at most two per path, so every position is below twice the round's paths
	uint32_t sp, lp;
	nee_append2(want_sun, want_light, cnt + 1, sp, lp);
	if (want_sun) {
		W.ox[sp] = sun_o.x; W.oy[sp] = sun_o.y; W.oz[sp] = sun_o.z;
		W.dx[sp] = sun_d.x; W.dy[sp] = sun_d.y; W.dz[sp] = sun_d.z;
		W.sx[i] = sun_x.x; W.sy[i] = sun_x.y; W.sz[i] = sun_x.z;
	}
	if (want_light) {
		W.ox[lp] = lo.x; W.oy[lp] = lo.y; W.oz[lp] = lo.z;
		W.dx[lp] = ld.x; W.dy[lp] = ld.y; W.dz[lp] = ld.z;
		W.lx[i] = lx.x; W.ly[i] = lx.y; W.lz[i] = lx.z;
		W.exp_surf[i] = exp_surf; W.exp_tri[i] = exp_tri;
	}
	if (i < n) {
		W.sun_pos[i] = want_sun ? (sp | (catcher_req ? kNeeCatcher : 0u)) : kNeeNone;
		W.light_pos[i] = want_light ? lp : kNeeNone;
	}
	const uint64_t lm = __ballot(want_light);
	if (lm != 0 && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)lm) - 1)) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + 2), (unsigned long long)__popcll(lm));
	// the continuation: a lane appends at most one entry, and a pending shadow catcher none here, so every position is below n
	uint32_t pos, unused;
	nee_append2(alive, false, cnt, pos, unused);
	if (alive) {
		out.ox[pos] = o.x; out.oy[pos] = o.y; out.oz[pos] = o.z;
		out.dx[pos] = d.x; out.dy[pos] = d.y; out.dz[pos] = d.z;
		out.tx[pos] = T.x; out.ty[pos] = T.y; out.tz[pos] = T.z; out.pp[pos] = p_prev;
		out.id[pos] = id; out.dp[pos] = (depth << 16) | pass;
	}
}

// The answers of the round's shadow rays (SH: their closest hits). One lane per path of the round, sun before light.
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
				visible = SH.surface[lp] == (int32_t)W.exp_surf[i] && SH.triangle[lp] == (int32_t)W.exp_tri[i];
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

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_nee_generate(const DevScene& S, const RenderParams& P, const NeeStream& out, float4* L, uint32_t n, hipStream_t stream) {
	hipLaunchKernelGGL(k_nee_generate, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, S, P, out, L, n);
	return hipGetLastError();
}

template <bool TEX, bool ALPHA>
static void nee_shade_sun(bool sun, dim3 grid, hipStream_t stream, const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeStream& in, const NeeHits& H, uint32_t n,
                          const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L) {
	if (sun) hipLaunchKernelGGL((k_nee_shade<TEX, ALPHA, true>), grid, dim3(kNeeBlock), 0, stream, S, P, Lt, in, H, n, out, W, cnt, L);
	else hipLaunchKernelGGL((k_nee_shade<TEX, ALPHA, false>), grid, dim3(kNeeBlock), 0, stream, S, P, Lt, in, H, n, out, W, cnt, L);
}

hipError_t launch_nee_shade(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeStream& in, const NeeHits& H, uint32_t n, const NeeStream& out,
                            const NeeShadow& W, uint32_t* cnt, float4* L, hipStream_t stream) {
	const dim3 grid((n + kNeeBlock - 1) / kNeeBlock);
	const bool sun = S.sun.present != 0;
	if (S.any_texture) {
		if (S.any_alpha) nee_shade_sun<true, true>(sun, grid, stream, S, P, Lt, in, H, n, out, W, cnt, L);
		else nee_shade_sun<true, false>(sun, grid, stream, S, P, Lt, in, H, n, out, W, cnt, L);
	} else {
		if (S.any_alpha) nee_shade_sun<false, true>(sun, grid, stream, S, P, Lt, in, H, n, out, W, cnt, L);
		else nee_shade_sun<false, false>(sun, grid, stream, S, P, Lt, in, H, n, out, W, cnt, L);
	}
	return hipGetLastError();
}

hipError_t launch_nee_settle(const NeeStream& in, uint32_t n, const NeeShadow& W, const NeeHits& SH, const NeeStream& out, uint32_t* cnt, float4* L, hipStream_t stream) {
	hipLaunchKernelGGL(k_nee_settle, dim3((n + kNeeBlock - 1) / kNeeBlock), dim3(kNeeBlock), 0, stream, in, n, W, SH, out, cnt, L);
	return hipGetLastError();
}

}  // namespace ptx
