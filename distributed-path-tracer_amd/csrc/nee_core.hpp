// The path vertex of ptx_render_nee (include/ptx.h has the estimator), shared by its two forms: k_nee_shade (nee.hip) loads the hit and the
// path state from the round's arrays and stores what nee_vertex returns; k_nee_fused (nee_fused.hip) calls it on registers.
// Numerics as in kernels.hip: IEEE binary32 in the written order, no contraction.
#pragma once
#include <utility>
#include "device_core.hpp"

namespace ptx {

// ---- the variant mask. What a scene and a call compile into the vertex is one uint32_t of these bits: the only template argument of a variant
// (V) from the kernels down to nee_candidate, the argument of nee_fused_block, and the index of the launchers' tables.
// Low four bits, the scene: TEX / ALPHA / SUN compile the texture lookups / the pass-through and catcher code / the sun request in, as the
// render variants do; ENV the environment sample (PTX_NEE_ENV_SAMPLES with a table; TEX only: a map implies the TEX variants).
// High three bits, the PART (V >> kNeePartShift): SPDF the weights of PTX_NEE_SAMPLER_PDF, RIS the light sample chosen among ris_m candidates
// (PTX_NEE_CANDIDATES), PUN punctual lights on the scene. nee_fused.hip is compiled once per part.
// One more PART bit, LTREE: a non-empty light list in tree mode (PTX_LIGHT_PICK_TREE): the triangle of a light sample comes from the light
// tree, and the path carries x_prev. k_nee_shade (nee.hip) and k_nee_fused (nee_fused.hip) have such variants, k_nee_fused_motion has
// none; they stand in a second list, kNeeTreeVariants.
enum : uint32_t { NEE_TEX = 1u, NEE_ALPHA = 2u, NEE_SUN = 4u, NEE_ENV = 8u, NEE_SPDF = 16u, NEE_RIS = 32u, NEE_PUN = 64u, NEE_LTREE = 128u };
constexpr uint32_t kNeePartShift = 4, kNeeSceneMask = (1u << kNeePartShift) - 1, kNeeParts = 8;

// The variants that exist, as data: every mask but those with ENV and without TEX, ascending, so 12 per part. The launchers' tables are built
// from this list and from nothing else; a mask that is not in it has no kernel.
constexpr uint32_t kNeeVariantCount = 96;
struct NeeVariantList { uint32_t v[kNeeVariantCount]; uint32_t n; };
constexpr NeeVariantList nee_variant_list() {
	NeeVariantList l{};
	for (uint32_t v = 0; v < (kNeeParts << kNeePartShift); v++) {
		if ((v & NEE_ENV) && !(v & NEE_TEX)) continue;
		if (l.n < kNeeVariantCount) l.v[l.n] = v;
		l.n++;
	}
	return l;
}
constexpr NeeVariantList kNeeVariants = nee_variant_list();
// whether `pred` holds for every entry of the list
template <typename Pred>
constexpr bool nee_all_variants(Pred pred) {
	for (uint32_t i = 0; i < kNeeVariantCount; i++)
		if (!pred(kNeeVariants.v[i])) return false;
	return true;
}
constexpr bool nee_env_has_tex(uint32_t v) { return !(v & NEE_ENV) || (v & NEE_TEX); }
static_assert(kNeeVariants.n == kNeeVariantCount, "96 variants: 12 scene masks in each of the 8 parts");
static_assert(nee_all_variants(nee_env_has_tex), "ENV reads the map through the TEX code");
// The tree variants, a second list beside the first: every entry of kNeeVariants with LTREE set, in its order
constexpr NeeVariantList nee_tree_variant_list() {
	NeeVariantList l = nee_variant_list();
	for (uint32_t i = 0; i < kNeeVariantCount; i++) l.v[i] |= NEE_LTREE;
	return l;
}
constexpr NeeVariantList kNeeTreeVariants = nee_tree_variant_list();

// The one rule from a scene and a call to a variant, for both forms. A table (Ev) means a map, and a map means the ENV variants, which are TEX
// variants: a scene without textures or without an environment texture cannot have one. sampler_pdf: SPDF. candidates > 1: RIS with
// M = candidates; ris_m is what the kernel receives. Pn.n != 0: PUN.
// Lt.n != 0 with a tree (Lt.nodes): LTREE (launch_nee_fused_motion has no kernel for it and refuses the mask).
inline hipError_t nee_select_variant(const DevScene& S, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, uint32_t& V, uint32_t& ris_m) {
	V = ((Lt.n != 0 && Lt.nodes != nullptr) ? NEE_LTREE : 0u) | (S.any_texture ? NEE_TEX : 0u) | (S.any_alpha ? NEE_ALPHA : 0u) | (S.sun.present != 0 ? NEE_SUN : 0u) | (sampler_pdf ? NEE_SPDF : 0u) | (candidates > 1 ? NEE_RIS : 0u) | (Pn.n != 0 ? NEE_PUN : 0u);
	ris_m = candidates > 1 ? candidates : 1u;
	if (Ev.row_cdf) {
		if (!S.any_texture || S.env_tex < 0) return hipErrorInvalidValue;
		V |= NEE_ENV;
	}
	return hipSuccess;
}

enum { BLOCK_LIGHT = 3, BLOCK_ENV = 4 };   // Philox blocks of the light sample's and the environment sample's draws (BLOCK_SURFACE / BLOCK_SUN / BLOCK_JITTER: device_core.hpp)
enum { BLOCK_PUNCTUAL = 0x200 };           // punctual lights on the scene: candidate j draws its strategy (x) and its light (y) from block BLOCK_PUNCTUAL + j
enum { BLOCK_RIS = 0x100 };                // PTX_NEE_CANDIDATES: candidate j draws from blocks BLOCK_LIGHT + 2 j and BLOCK_ENV + 2 j, selection j from component j & 3 of block BLOCK_RIS + (j >> 2)

// sample id within the pass (sample-major, pixel-minor) -> image pixel and global sample index, as k_render_pass enumerates them
DEV void nee_sample_of(const RenderParams& P, uint32_t id, uint32_t& px, uint32_t& py, uint32_t& sample) {
	const uint32_t s_local = id / P.n_pixels;
	uint32_t p_local = id - s_local * P.n_pixels;
	if (P.pixels) p_local = P.pixels[p_local];
	px = P.x0 + p_local % P.w; py = P.y0 + p_local / P.w;
	sample = P.sample0 + s_local;
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

// ---- the environment map as a light (PTX_NEE_ENV_SAMPLES; include/ptx.h has the table and the pdf)
// (u, v) of the miss lookup for direction d, and the table's box (i, j) they fall into
DEV void env_box(const NeeEnv& E, V3 d, float& u, float& v, uint32_t& i, uint32_t& j) {
	u = atan2f(d.z, d.x) * 0.1591F + 0.5F;
	v = asinf(d.y) * 0.3183F + 0.5F;
	const uint32_t bi = (uint32_t)(u * (float)E.w), bj = (uint32_t)((1 - v) * (float)E.h);
	i = bi < E.w - 1 ? bi : E.w - 1;
	j = bj < E.h - 1 ? bj : E.h - 1;
}
// solid-angle density with which the environment sample produces a direction d of box (i, j): the box's probability as the STORED
// float32 tables give it (what the sampler realises), over the box's solid angle
DEV float env_pdf_box(const NeeEnv& E, V3 d, uint32_t i, uint32_t j) {
	const float c = sqrt_exact(pmax(0.0f, 1 - d.y * d.y));
	if (!(c > 0)) return 0.0f;
	const float* row = E.cell_cdf + (size_t)j * E.w;
	const float pr = E.row_cdf[j] - (j ? E.row_cdf[j - 1] : 0.0f), pc = row[i] - (i ? row[i - 1] : 0.0f);
	const float Pb = pr * pc;
	return ((Pb * (float)(E.w * E.h)) * (0.1591F * 0.3183F)) / c;
}
DEV float env_pdf(const NeeEnv& E, V3 d) {
	float u, v;
	uint32_t i, j;
	env_box(E, d, u, v, i, j);
	return env_pdf_box(E, d, i, j);
}
// first entry of cdf[0 .. n) with x < cdf[entry], clamped to n - 1
DEV uint32_t env_pick(const float* __restrict__ cdf, uint32_t n, float x) {
	uint32_t a = 0, b = n;
	while (a < b) {
		const uint32_t mid = a + (b - a) / 2;
		if (x < cdf[mid]) b = mid; else a = mid + 1;
	}
	return a < n - 1 ? a : n - 1;
}

// ---- the density of LIB's BSDF sampler (PTX_NEE_SAMPLER_PDF; include/ptx.h has the derivation)
// Solid-angle density with which importance_sample produces direction w at a vertex: the GGX half-vector density D(h) (n.h) / (4 (o.h)) of
// the specular draw and the cosine density of the diffuse draw, mixed as the draw rnd.y < spec_prob mixes them. roughness is the clamped one
// importance_sample receives. pdf_specular, LIB's pdf VALUE, is not this density; pdf_diffuse is.
DEV float sampler_pdf(V3 normal, V3 outcoming, V3 w, float roughness, float spec_prob) {
	const float a = roughness * roughness, a2 = a * a;
	const V3 hv = outcoming + w;
	const V3 h = hv / sqrt_exact(dot(hv, hv));
	const float nh = dot(normal, h), oh = dot(outcoming, h);
	const float t = (nh * nh) * (a2 - 1) + 1;
	const float ps_spec = (nh > 0 && oh > 0) ? (a2 * nh) / ((((float)kPi * t) * t) * (4 * oh)) : 0.0f;
	return lerpf(pdf_diffuse(normal, w), ps_spec, spec_prob);
}

// ---- punctual lights (include/ptx.h: PUNCTUAL LIGHTS, PUNCTUAL PICK)
// Light k seen from x, the expressions of PUNCTUAL SAMPLE: v, dist2, dist, w, att and the range test. One function for the sample and for a
// leaf's importance, so that the importance is 0 exactly where the sample's own geometric conditions fail. false: dist2 is not > 0, and
// nothing but dist2 is written.
DEV bool punctual_geom(const NeePunctual& Pn, uint32_t k, V3 x, V3& w, float& dist2, float& dist, float& att, bool& in_range) {
	const float4 r0 = Pn.recs[4 * (size_t)k], r1 = Pn.recs[4 * (size_t)k + 1];
	const V3 v = mk(r0.x, r0.y, r0.z) - x;
	dist2 = dot(v, v);
	if (!(dist2 > 0)) return false;
	dist = sqrt_exact(dist2);
	w = v / dist;
	att = 1.0f;
	if (r1.w != 0.0f) {   // a spot: the cone's smooth edge
		const float4 r2 = Pn.recs[4 * (size_t)k + 2], r3 = Pn.recs[4 * (size_t)k + 3];
		const float cd = dot(mk(r1.x, r1.y, r1.z), -w);
		const float sm = clampf((cd - r3.x) / pmax(r2.w - r3.x, 1e-6F), 0, 1);
		att = sm * sm;
	}
	in_range = r0.w == 0.0f || dist <= r0.w;
	return true;
}
constexpr uint32_t kPunctualLeaf = 0x80000000u;   // word 7 of a tree node: a leaf, the light's index in the low bits
// importance of the node (n0, n1) seen from x: power / max(squared distance to the box's centre, squared half diagonal) for a branch, the
// light's own power * att / dist2 for a leaf
DEV float punctual_importance(const NeePunctual& Pn, float4 n0, float4 n1, V3 x) {
	const uint32_t w7 = __float_as_uint(n1.w);
	if (w7 & kPunctualLeaf) {
		V3 w;
		float dist2, dist, att;
		bool in_range;
		if (!punctual_geom(Pn, w7 & ~kPunctualLeaf, x, w, dist2, dist, att, in_range) || !in_range) return 0.0f;
		return (n0.w * att) / dist2;
	}
	const V3 lo = mk(n0.x, n0.y, n0.z), hi = mk(n1.x, n1.y, n1.z);
	const V3 c = (lo + hi) * 0.5F, d = x - c, h = (hi - lo) * 0.5F;
	return n0.w / pmax(dot(d, d), dot(h, h));
}
// The stochastic descent from the root: at a branch the two children (adjacent nodes: one 64-byte read) are weighed from x, u picks one and
// is stretched back to [0, 1). -> the leaf's light; pmf: the product of the branch probabilities as the descent realised them. The tree is
// balanced by count, so the trip counts of a wave's lanes differ by one at most.
DEV uint32_t punctual_pick_tree(const NeePunctual& Pn, V3 x, float u, float& pmf) {
	pmf = 1.0f;
	uint32_t w7 = __float_as_uint(Pn.nodes[1].w);
	while (!(w7 & kPunctualLeaf)) {
		const float4* __restrict__ ch = Pn.nodes + 2 * (size_t)w7;
		const float4 l0 = ch[0], l1 = ch[1], r0 = ch[2], r1 = ch[3];
		const float il = punctual_importance(Pn, l0, l1, x), ir = punctual_importance(Pn, r0, r1, x);
		const float s = il + ir;
		const float p = (s > 0 && s < __builtin_inff()) ? il / s : 0.5F;
		if (u < p) {
			pmf = pmf * p;
			u = u / p;
			w7 = __float_as_uint(l1.w);
		} else {
			const float q1 = 1 - p;
			pmf = pmf * q1;
			u = (u - p) / q1;
			w7 = __float_as_uint(r1.w);
		}
		u = pmin(u, 0x1.fffffep-1F);
	}
	return w7 & ~kPunctualLeaf;
}
// Which light a punctual candidate samples and the probability pmf_k that divides it: the tree's descent from x when the scene has one
// (a wave-uniform test of a kernel argument), else the first entry of the CDF with u below it and the difference of the STORED entries
DEV uint32_t punctual_pick(const NeePunctual& Pn, V3 x, float u, float& pmf) {
	if (Pn.nodes) return punctual_pick_tree(Pn, x, u, pmf);
	const uint32_t k = env_pick(Pn.cdf, Pn.n, u);
	pmf = Pn.cdf[k] - (k ? Pn.cdf[k - 1] : 0.0f);   // from the stored values: what the pick realises
	return k;
}

// ---- the light tree over the light list (include/ptx.h: LIGHT PICK)
constexpr uint32_t kLightLeaf = 0x80000000u;   // word 7 of a tree node: a leaf, the list entry in the low bits
// importance of the node (n0, n1) seen from x, one formula for leaves and branches: power / max(squared distance to the box's centre,
// squared half diagonal)
DEV float light_importance(float4 n0, float4 n1, V3 x) {
	const V3 lo = mk(n0.x, n0.y, n0.z), hi = mk(n1.x, n1.y, n1.z);
	const V3 c = (lo + hi) * 0.5F, d = x - c, h = (hi - lo) * 0.5F;
	return n0.w / pmax(dot(d, d), dot(h, h));
}
// The probability p of going left at the branch whose left child is node `left`, seen from x; wl, wr: word 7 of the two children (adjacent
// nodes: one 64-byte read). Shared by the stochastic pick and the directed pmf, so that the two multiply the same numbers.
DEV float light_branch_p(const NeeLights& Lt, uint32_t left, V3 x, uint32_t& wl, uint32_t& wr) {
	const float4* __restrict__ ch = Lt.nodes + 2 * (size_t)left;
	const float4 l0 = ch[0], l1 = ch[1], r0 = ch[2], r1 = ch[3];
	const float il = light_importance(l0, l1, x), ir = light_importance(r0, r1, x);
	const float s = il + ir;
	wl = __float_as_uint(l1.w); wr = __float_as_uint(r1.w);
	return (s > 0 && s < __builtin_inff()) ? il / s : 0.5F;
}
// The stochastic descent from the root (punctual_pick_tree's loop): -> the leaf's list entry; pmf: the product of the branch probabilities
// as the descent realised them. The tree is balanced by count, so the trip counts of a wave's lanes differ by one at most.
DEV uint32_t light_pick_tree(const NeeLights& Lt, V3 x, float u, float& pmf) {
	pmf = 1.0f;
	uint32_t w7 = __float_as_uint(Lt.nodes[1].w);
	while (!(w7 & kLightLeaf)) {
		uint32_t wl, wr;
		const float p = light_branch_p(Lt, w7, x, wl, wr);
		if (u < p) {
			pmf = pmf * p;
			u = u / p;
			w7 = wl;
		} else {
			const float q1 = 1 - p;
			pmf = pmf * q1;
			u = (u - p) / q1;
			w7 = wr;
		}
		u = pmin(u, 0x1.fffffep-1F);
	}
	return w7 & ~kLightLeaf;
}
// pmf_k(x): the same loop from the root, taking at step i the side bit i of path[k] names and multiplying the same p or 1 - p in the same
// order: bit for bit the pmf light_pick_tree returns whenever it returns k
DEV float light_pmf_tree(const NeeLights& Lt, uint32_t k, V3 x) {
	float pmf = 1.0f;
	uint32_t word = Lt.path[k];
	uint32_t w7 = __float_as_uint(Lt.nodes[1].w);
	while (!(w7 & kLightLeaf)) {
		uint32_t wl, wr;
		const float p = light_branch_p(Lt, w7, x, wl, wr);
		if (!(word & 1u)) {
			pmf = pmf * p;
			w7 = wl;
		} else {
			const float q1 = 1 - p;
			pmf = pmf * q1;
			w7 = wr;
		}
		word >>= 1;
	}
	return pmf;
}
// first entry of the list's CDF with u below it, clamped to the last: the CDF mode's pick
DEV uint32_t light_pick_cdf(const NeeLights& Lt, float u) {
	uint32_t a = 0, b = Lt.n;
	while (a < b) {
		const uint32_t mid = a + (b - a) / 2;
		if (u < Lt.cdf[mid]) b = mid; else a = mid + 1;
	}
	return a < Lt.n - 1 ? a : Lt.n - 1;
}
// The pick and the directed pmf in the scene's mode (the batch calls): the tree's when the scene has one, else the CDF's with the
// difference of the STORED entries
DEV uint32_t light_pick(const NeeLights& Lt, V3 x, float u, float& pmf) {
	if (Lt.nodes) return light_pick_tree(Lt, x, u, pmf);
	const uint32_t k = light_pick_cdf(Lt, u);
	pmf = Lt.cdf[k] - (k ? Lt.cdf[k - 1] : 0.0f);
	return k;
}
DEV float light_pmf(const NeeLights& Lt, uint32_t k, V3 x) {
	if (Lt.nodes) return light_pmf_tree(Lt, k, x);
	return Lt.cdf[k] - (k ? Lt.cdf[k - 1] : 0.0f);
}

// What a vertex leaves besides the path state: whether the path goes on, and its up-to-two shadow requests
struct NeeVertex {
	bool alive = false;         // the path continues with (o, d, T, p_prev, depth, pass) as the vertex left them
	bool want_sun = false;      // sun ray (sun_o, sun_d): unoccluded adds sun_x = T * direct_out ...
	bool catcher_req = false;   // ... or, a shadow catcher's: unoccluded lets the path through from sun_x, occluded ends it
	bool want_light = false;    // light ray (lo, ld): lx is added iff its closest hit is triangle exp_tri of surface exp_surf (kNeeEnvRay: iff it hits nothing)
	V3 sun_o = {0, 0, 0}, sun_d = {0, 0, 1}, sun_x = {0, 0, 0}, lo = {0, 0, 0}, ld = {0, 0, 1}, lx = {0, 0, 0};
	uint32_t exp_surf = 0, exp_tri = 0;
};

// One candidate light sample of a vertex (include/ptx.h: LIGHT SAMPLE, and SELECTION / ENVIRONMENT SAMPLE with ENV, ps with SPDF), drawn from the
// Philox blocks block_light / block_env: the vertex's position and frame, its material terms and T before its update. A candidate that
// contributes sets `want`; then lx is its x, (lo, ld) its shadow ray and (exp_surf, exp_tri) its visibility rule. Otherwise nothing is written.
// The unflagged vertex takes one, from BLOCK_LIGHT / BLOCK_ENV, straight into its NeeVertex — `want` is set in place, not returned: the
// statements are then the former ones, and the unflagged kernels keep their registers. The RIS vertex takes M of them.
// PUN (punctual lights on the scene, Pn; include/ptx.h: PUNCTUAL LIGHTS): the candidate is a punctual sample with probability c_p, drawn from
// block_pun, and the other strategies' densities carry (1 - c_p). Without PUN, Pn, c_p and block_pun are not read and no statement changes.
// Its light and pmf come from punctual_pick: the CDF's, or with a light tree on the scene (Pn.nodes) the descent from the vertex's position.
// LTREE (a non-empty list in tree mode; include/ptx.h: LIGHT PICK): the triangle and pmf_i come from light_pick_tree at the vertex's position,
// and p_l is (pmf_i * dist2) / (cg * A_i). Without LTREE the tree is not read and no statement changes.
template <uint32_t V>
DEV void nee_candidate(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, float c_env, uint32_t pixel, uint32_t sample, uint32_t depth, uint32_t pass,
                       uint32_t block_light, uint32_t block_env, const Surf& sf, V3 normal, V3 outcoming, V3 T, const MatEval& me, float roughness, float spec_prob, V3& lx, V3& lo, V3& ld,
                       uint32_t& exp_surf, uint32_t& exp_tri, bool& want, const NeePunctual& Pn = NeePunctual{}, float c_p = 0.0f, uint32_t block_pun = 0u) {
	constexpr bool TEX = (V & NEE_TEX) != 0, ENV = (V & NEE_ENV) != 0, SPDF = (V & NEE_SPDF) != 0, PUN = (V & NEE_PUN) != 0, LTREE = (V & NEE_LTREE) != 0;   // ALPHA, SUN and RIS are not read here
	if constexpr (PUN) {
		const float4 q = draws(P, pixel, sample, depth, pass, block_pun);
		if (c_p == 1.0F || q.x < 0.5F) {
			float pmf;
			const uint32_t k = punctual_pick(Pn, sf.pos, q.y, pmf);
			V3 w;
			float dist2, dist, att;
			bool in_range;
			if (punctual_geom(Pn, k, sf.pos, w, dist2, dist, att, in_range)) {
				const float4 r2 = Pn.recs[4 * (size_t)k + 2];
				const V3 E = (mk(r2.x, r2.y, r2.z) * att) / dist2;
				if (dot(normal, w) > 0 && pmf > 0 && in_range && att > 0 && pmax(E.x, pmax(E.y, E.z)) > 0) {
					float pdf;
					const V3 brdf = eval_brdf(normal, outcoming, w, me.albedo, roughness, me.metallic, spec_prob, pdf);
					const float pe = pmax(pdf, kEps);
					const V3 qv = brdf / pe;
					const V3 qc = mk(clampf(qv.x, 0, 1), clampf(qv.y, 0, 1), clampf(qv.z, 0, 1));
					const V3 b = qc * pe;   // LIB's integrand at w, cosine included
					lx = ((T * b) * E) / (c_p * pmf);
					lo = sf.pos + w * kEps;
					ld = w;
					exp_surf = kNeePunctualRay; exp_tri = __float_as_uint(dist);
					want = true;
				}
			}
			return;
		}
	}
	bool to_env = false;
	if constexpr (ENV) {
		to_env = Lt.n == 0 || draws(P, pixel, sample, depth, pass, block_light).w < 0.5F;
		if (to_env) {
			const float4 q = draws(P, pixel, sample, depth, pass, block_env);
			const uint32_t j = env_pick(Ev.row_cdf, Ev.h, q.x);
			const uint32_t i = env_pick(Ev.cell_cdf + (size_t)j * Ev.w, Ev.w, q.y);
			const float u = ((float)i + q.z) / (float)Ev.w, v = 1 - ((float)j + q.w) / (float)Ev.h;
			const float phi = (u - 0.5F) / 0.1591F, lat = (v - 0.5F) / 0.3183F;
			const float cl = cosf(lat);
			const V3 w = mk(cl * cosf(phi), sinf(lat), cl * sinf(phi));
			float fu, fv;
			uint32_t fi, fj;
			env_box(Ev, w, fu, fv, fi, fj);   // the lookup's own (u, v): a sample it maps to another box is dropped, so the pdf stays a function of direction
			if (fi == i && fj == j && dot(normal, w) > 0) {
				const float p = env_pdf_box(Ev, w, fi, fj);
				const float4 e = tex_sample(S, S.env_tex, fu, fv);
				const V3 Le = mk(e.x, e.y, e.z) * mk(P.env[0], P.env[1], P.env[2]);
				if (p > 0 && pmax(Le.x, pmax(Le.y, Le.z)) > 0) {
					float pdf;
					const V3 brdf = eval_brdf(normal, outcoming, w, me.albedo, roughness, me.metallic, spec_prob, pdf);
					const float pe = pmax(pdf, kEps);
					const V3 qv = brdf / pe;
					const V3 qc = mk(clampf(qv.x, 0, 1), clampf(qv.y, 0, 1), clampf(qv.z, 0, 1));
					float pw = pe;
					if constexpr (SPDF) pw = sampler_pdf(normal, outcoming, w, roughness, spec_prob);
					if (!SPDF || pw > 0) {   // a direction the BSDF sampler cannot produce carries nothing
						float p_e = c_env * p;
						if constexpr (PUN) p_e = (1 - c_p) * p_e;
						const float wl = pw / (pw + p_e);
						lx = ((T * qc) * wl) * Le;
						lo = sf.pos + w * kEps;
						ld = w;
						exp_surf = kNeeEnvRay; exp_tri = 0;
						want = true;
					}
				}
			}
		}
	}
	if (Lt.n != 0 && !to_env) {
		const float4 r = draws(P, pixel, sample, depth, pass, block_light);
		uint32_t k;
		float pmf_i = 1.0f;
		if constexpr (LTREE) {
			k = light_pick_tree(Lt, sf.pos, r.x, pmf_i);
		} else {
			uint32_t a = 0, b = Lt.n;   // first entry with r.x < cdf
			while (a < b) {
				const uint32_t mid = a + (b - a) / 2;
				if (r.x < Lt.cdf[mid]) b = mid; else a = mid + 1;
			}
			k = a < Lt.n - 1 ? a : Lt.n - 1;
		}
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
			if (dot(normal, w) > 0 && dot(n_y, -w) > 0 && cg > 0 && pmax(Le.x, pmax(Le.y, Le.z)) > 0 && (!LTREE || pmf_i > 0)) {
				float pdf;
				const V3 brdf = eval_brdf(normal, outcoming, w, me.albedo, roughness, me.metallic, spec_prob, pdf);
				const float pe = pmax(pdf, kEps);
				const V3 q = brdf / pe;
				const V3 qc = mk(clampf(q.x, 0, 1), clampf(q.y, 0, 1), clampf(q.z, 0, 1));
				float p_l;
				if constexpr (LTREE) p_l = (pmf_i * dist2) / (cg * g.w);
				else p_l = dist2 / (cg * Lt.area);
				if constexpr (ENV) p_l = (1 - c_env) * p_l;
				if constexpr (PUN) p_l = (1 - c_p) * p_l;
				float pw = pe;
				if constexpr (SPDF) pw = sampler_pdf(normal, outcoming, w, roughness, spec_prob);
				if (!SPDF || pw > 0) {
					const float wl = pw / (pw + p_l);
					lx = ((T * qc) * wl) * Le;
					lo = sf.pos + w * kEps;
					ld = w;
					exp_surf = lt.x; exp_tri = lt.y;
					want = true;
				}
			}
		}
	}
}

// One vertex of one path. The hit: surface (< 0: miss), triangle within the surface's mesh, barycentrics b1, b2 and the world distance, as the
// scene's intersect route reports them. TEX / ALPHA / SUN compile the texture lookups / the pass-through and catcher code / the sun request
// in, as the render variants do. The statements are shade_vertex<SUN, ALPHA, TEX, false>'s, in its order, with the emission weighted and the
// light sample taken before the BSDF sample. Returns whether L received a term (the record-based form stores its record then).
// ENV (PTX_NEE_ENV_SAMPLES with a table, Ev): the light sample may go towards the environment map, and the map's radiance on a miss is weighted
// against that sample. Without ENV, Ev is not read and the statements are the unflagged estimator's.
// SPDF (PTX_NEE_SAMPLER_PDF): sampler_pdf takes pe's place in the two wl and in p_prev, and nowhere else. Without SPDF no statement changes.
// RIS (PTX_NEE_CANDIDATES(m), m > 1): the light sample is chosen among ris_m candidates. Without RIS ris_m is not read and no statement changes.
// PUN (punctual lights on the scene, Pn): a candidate may be a punctual sample, and the other strategies' densities carry (1 - c_p) in every
// weight. Without PUN, Pn is not read and no statement changes.
// LTREE (a non-empty list in tree mode): the emission weight's density is the directed pmf of the hit triangle seen from *x_prev, the position
// of the vertex that drew the BSDF sample, and x_prev is set where p_prev is set. Without LTREE x_prev is not touched (nullptr).
template <uint32_t V>
DEV bool nee_vertex(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, uint32_t ris_m, uint32_t pixel, uint32_t sample, int32_t surf, uint32_t tri, float b1, float b2,
                    float hit_dist, V3& o, V3& d, V3& T, V3& L, float& p_prev, uint32_t& depth, uint32_t& pass, NeeVertex& out, const NeePunctual& Pn = NeePunctual{},
                    bool moved = false, const XformRecs& Xm = XformRecs{}, V3* x_prev = nullptr) {
	constexpr bool TEX = (V & NEE_TEX) != 0, ALPHA = (V & NEE_ALPHA) != 0, SUN = (V & NEE_SUN) != 0, ENV = (V & NEE_ENV) != 0;
	constexpr bool SPDF = (V & NEE_SPDF) != 0, RIS = (V & NEE_RIS) != 0, PUN = (V & NEE_PUN) != 0, LTREE = (V & NEE_LTREE) != 0;
	bool& alive = out.alive;
	bool& want_sun = out.want_sun;
	bool& want_light = out.want_light;
	bool& catcher_req = out.catcher_req;
	V3 &sun_o = out.sun_o, &sun_d = out.sun_d, &sun_x = out.sun_x, &lo = out.lo, &ld = out.ld, &lx = out.lx;
	uint32_t &exp_surf = out.exp_surf, &exp_tri = out.exp_tri;
	bool store = false;
	const float c_env = (ENV && Lt.n != 0) ? 0.5F : 1.0F;   // share of the vertices whose light sample goes to the map (ENV only)
	const float c_p = (ENV || Lt.n != 0) ? 0.5F : 1.0F;     // share of the candidates that are punctual samples (PUN only): all of them when no other strategy exists
	do {
		if (surf < 0) {   // miss: environment
			V3 env = mk(P.env[0], P.env[1], P.env[2]);
			if constexpr (TEX) {
				if (S.env_tex >= 0) {
					const float4 e = tex_sample(S, S.env_tex, atan2f(d.z, d.x) * 0.1591F + 0.5F, asinf(d.y) * 0.3183F + 0.5F);
					env = mk(e.x, e.y, e.z) * env;
				}
			}
			V3 add = T * env;
			if constexpr (ENV) {   // a BSDF-sampled direction that the environment sample of the previous vertex could have produced
				if (depth != 0 && pass == 0) {
					float p_e = c_env * env_pdf(Ev, d);
					if constexpr (PUN) p_e = (1 - c_p) * p_e;
					add = add * (p_prev / (p_prev + p_e));
				}
			}
			L = L + add;
			store = true;
			break;
		}
		const ShadeRec& R = S.shade[surf];
		Surf sf;
		// moved (the unfused kernels under active motion alone): the hit surface's model moves, and Xm holds its records at the path's time
		if (moved) hit_attributes_at(S, Xm.basis, Xm.origin, Xm.nmat, tri + S.surfaces[surf].tri_base, b1, b2, sf);
		else hit_attributes(S, R, tri + S.surfaces[surf].tri_base, b1, b2, sf);
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
				if (catcher) {   // the answer decides between the pass-through and the end of the path
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
				const float dist = hit_dist;
				float p_l;
				if constexpr (LTREE) p_l = (light_pmf_tree(Lt, (uint32_t)k, *x_prev) * (dist * dist)) / (cg * g.w);
				else p_l = (dist * dist) / (cg * Lt.area);
				if constexpr (ENV) p_l = (1 - c_env) * p_l;
				if constexpr (PUN) p_l = (1 - c_p) * p_l;
				em = em * (p_prev / (p_prev + p_l));
			}
		}
		L = L + em;
		store = true;
		if (last) break;
		// ---- light sample
		if constexpr (!RIS) {
			nee_candidate<V>(S, P, Lt, Ev, c_env, pixel, sample, depth, pass, BLOCK_LIGHT, BLOCK_ENV, sf, normal, outcoming, T, me, roughness, spec_prob, lx, lo, ld,
			                                   exp_surf, exp_tri, want_light, Pn, c_p, BLOCK_PUNCTUAL);
		} else {
			// M candidates, one kept by weighted reservoir selection (include/ptx.h: PTX_NEE_CANDIDATES). The reservoir is lx, ld, the visibility
			// rule, wsum and the chosen weight; lo follows from ld.
			float wsum = 0, w_y = 0;
			for (uint32_t j = 0; j < ris_m; j++) {
				V3 cx = {0, 0, 0}, co = {0, 0, 0}, cd = {0, 0, 1};
				uint32_t cs = 0, ct = 0;
				bool cw = false;
				nee_candidate<V>(S, P, Lt, Ev, c_env, pixel, sample, depth, pass, BLOCK_LIGHT + 2 * j, BLOCK_ENV + 2 * j, sf, normal, outcoming, T, me, roughness, spec_prob, cx, co, cd,
				                                   cs, ct, cw, Pn, c_p, BLOCK_PUNCTUAL + j);
				if (!cw) continue;
				const float w_j = pmax(cx.x, pmax(cx.y, cx.z));
				if (!(w_j > 0 && w_j < __builtin_inff())) continue;
				wsum = wsum + w_j;
				bool take = !want_light;   // the first kept candidate is chosen outright
				if (!take) {
					const float4 u4 = draws(P, pixel, sample, depth, pass, BLOCK_RIS + (j >> 2));
					const uint32_t c = j & 3u;
					const float u = c == 0 ? u4.x : c == 1 ? u4.y : c == 2 ? u4.z : u4.w;
					take = u * wsum < w_j;
				}
				if (take) { lx = cx; ld = cd; exp_surf = cs; exp_tri = ct; w_y = w_j; }
				want_light = true;
			}
			if (want_light) {
				lx = lx * ((wsum / (float)ris_m) / w_y);
				lo = sf.pos + ld * kEps;
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
		if constexpr (SPDF) {
			const float ps = sampler_pdf(normal, outcoming, inc, roughness, spec_prob);
			if (ps > 0 && ps < __builtin_inff()) p_prev = ps;
		}
		if constexpr (LTREE) *x_prev = sf.pos;
		o = sf.pos + inc * kEps;
		d = normalize(inc);
		depth++;
		pass = 0;
		alive = depth != P.bounces;
	} while (false);
	return store;
}

}  // namespace ptx
