// First-hit guide buffers for a denoiser (ptx_render_aov): mean albedo, world shading normal, depth and coverage of what each camera
// sample sees. The camera samples are ptx_render's (camera_ray, same Philox keys); the closest hits come from the scene's own intersect
// route (launch_intersect / launch_wf_intersect, issued by ptx_api.cpp between the kernels of this file), so they are bitwise the
// integrator's on every route. This file holds the three small kernels around them:
//   k_aov_generate   sample id -> (pixel, sample) -> camera ray, SoA of floats (the layout the intersect launches read)
//   k_aov_shade      one sample per lane: hit attributes, material lookups, the opacity draw of renderer.cpp:466-472 with the integrator's
//                    own draw (depth 0, BLOCK_SURFACE, lane x). The first vertex that does not pass through is the sample's surface: its
//                    two float4 records are stored by sample id. Samples that pass through are appended densely to the next round's stream
//                    (wave ballot + lane prefix count, one atomic per wave)
//   k_aov_resolve    adds a pixel's records in sample order into the caller's buffers (sums, bitwise reproducible, no float atomics)
// ptx_render_motion walks the same samples through the same body (aov_shade_sample) and records, in place of the two guide records, where
// the sample's surface point was on the previous frame's screen (k_aov_motion_shade); k_aov_resolve adds those records up as well.
// ptx_render_emission does the same with what the integrator adds at that surface: its emission, when the surface faces the ray
// (k_aov_emission_shade).
// Numerics as in kernels.hip: IEEE binary32 in the reference's operation order, no contraction.
#include "device_core.hpp"

namespace ptx {

constexpr int kAovBlock = 256;

// sample id within the pass (sample-major, pixel-minor) -> image pixel and global sample index, as k_render_pass enumerates them
DEV void aov_sample_of(const RenderParams& P, uint32_t id, uint32_t& px, uint32_t& py, uint32_t& sample) {
	const uint32_t s_local = id / P.n_pixels;
	uint32_t p_local = id - s_local * P.n_pixels;
	if (P.pixels) p_local = P.pixels[p_local];   // interleaved tile sharding: the pass covers a subset of the tile's pixels
	px = P.x0 + p_local % P.w; py = P.y0 + p_local / P.w;
	sample = P.sample0 + s_local;
}

// camera samples 0 .. n-1 of the pass -> stream entries 0 .. n-1 (scene::camera::get_ray; renderer.cpp:359-370)
__global__ void __launch_bounds__(kAovBlock) k_aov_generate(DevScene S0, RenderParams P, AovStream out, uint32_t n, RenderMotion Rm) {
	const uint32_t i = blockIdx.x * kAovBlock + threadIdx.x;
	if (i >= n) return;
	uint32_t px, py, sample;
	aov_sample_of(P, i, px, py, sample);
	DevScene S = S0;
	if (Rm.camera_moved) camera_at(S, Rm, sample_time(P, Rm, py * P.W + px, sample));   // the camera of the sample's own time (wave-uniform test)
	V3 o, d;
	camera_ray(S, P, px, py, sample, o, d);
	out.ox[i] = o.x; out.oy[i] = o.y; out.oz[i] = o.z;
	out.dx[i] = d.x; out.dy[i] = d.y; out.dz[i] = d.z;
}

// project(cam, p) of ptx_render_motion (include/ptx.h): the pixel coordinates at which the pinhole camera sees the world point p; false
// when p is not in front of it. The inverse of camera_get_ray for a basis that is a rotation times a uniform scale.
DEV bool motion_project(const float* origin, const float* basis, float tan_half_fov, const RenderParams& P, V3 p, float& fx, float& fy) {
	const V3 q = p - mk(origin[0], origin[1], origin[2]);
	const float cx = dot(mk(basis[0], basis[1], basis[2]), q), cy = dot(mk(basis[3], basis[4], basis[5]), q), cz = dot(mk(basis[6], basis[7], basis[8]), q);
	const float iz = 0 - cz;
	const float ratio = (float)P.W / (float)P.H;
	const float ndc_x = ((cx / iz) / ratio) / tan_half_fov, ndc_y = (cy / iz) / tan_half_fov;
	fx = ((ndc_x + 1) * 0.5F) * (float)P.W;
	fy = ((1 - ndc_y) * 0.5F) * (float)P.H;
	return cz < 0;
}

// The motion record of a sample that ends on `surf` at `pos` (hit_attributes' position; its local point is recomputed from the same
// corners with the same operations): (previous - current pixel position, distance from the previous camera, 1), or zeros when either
// camera does not have the point in front of it.
DEV float4 motion_record(const DevScene& S, const RenderParams& P, const AovMotion& Mo, int32_t surf, uint32_t tri_word, float b1, float b2, V3 pos) {
	V3 pos_prev = pos;
	const uint32_t m = S.surfaces[surf].model;
	if (Mo.prev_xform && Mo.moved[m]) {
		const float b0 = 1 - b1 - b2;
		const float4* T = S.tris + 9 * (size_t)(tri_word & S.tri_id_mask);
		const float4 A = T[0], B = T[1], C = T[2];
		const V3 lp = mk(A.x, A.y, A.z) * b0 + mk(B.x, B.y, B.z) * b1 + mk(C.x, C.y, C.z) * b2;
		const float* x = Mo.prev_xform + 12 * (size_t)m;   // origin, then the basis' columns
		pos_prev = mulmv(x + 3, lp) + mk(x[0], x[1], x[2]);
	}
	float cx, cy, qx, qy;
	const bool cur = motion_project(S.cam.origin, S.cam.basis, S.cam.tan_half_fov, P, pos, cx, cy);
	const bool prv = motion_project(Mo.origin, Mo.basis, Mo.tan_half_fov, P, pos_prev, qx, qy);
	if (!(cur && prv)) return make_float4(0.f, 0.f, 0.f, 0.f);
	return make_float4(qx - cx, qy - cy, length(pos_prev - mk(Mo.origin[0], Mo.origin[1], Mo.origin[2])), 1.0f);
}

// What a sample's surface is recorded as: the two guide records, or ONE record (rec[id]) of motion or of emission.
enum : int { AOV_GUIDES = 0, AOV_MOTION = 1, AOV_EMISSION = 2 };

// One vertex of every live sample. TEX / ALPHA compile the texture lookups / the pass-through in, as the render variants do.
template <bool TEX, bool ALPHA, int KIND>
DEV void aov_shade_sample(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* __restrict__ n_out,
                          float4* __restrict__ rec, size_t rec_stride, const AovMotion* Mo, const RenderMotion* Rm = nullptr) {
	const uint32_t i = blockIdx.x * kAovBlock + threadIdx.x;
	bool through = false;
	V3 o = {0, 0, 0}, d = {0, 0, 1};
	uint32_t id = 0, pass = 0;
	if (i < n) {
		id = in.id ? in.id[i] : i;
		if constexpr (ALPHA) pass = in.id ? in.pass[i] : 0u;
		float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rn = ra;   // a miss adds nothing
		const int32_t surf = H.surface[i];
		if (surf >= 0) {
			const ShadeRec& R = S.shade[surf];
			Surf sf;
			// active motion (the guide kernels alone; a wave-uniform test of a kernel argument): the sample's time, and the records of a moving
			// model's surface at that time
			float u = 0;
			bool moved = false;
			XformRecs Xm;
			if (Rm && Rm->active) {
				uint32_t tx, ty, tsample;
				aov_sample_of(P, id, tx, ty, tsample);
				u = sample_time(P, *Rm, ty * P.W + tx, tsample);
				if (Rm->models_moved) {
					const uint32_t m = S.surfaces[surf].model;
					moved = Rm->models.moved[m] != 0u;
					if (moved) model_records_at(Rm->models, m, u, Xm);
				}
			}
			if (moved) hit_attributes_at(S, Xm.basis, Xm.origin, Xm.nmat, (uint32_t)H.triangle[i] + S.surfaces[surf].tri_base, H.b1[i], H.b2[i], sf);
			else hit_attributes(S, R, (uint32_t)H.triangle[i] + S.surfaces[surf].tri_base, H.b1[i], H.b2[i], sf);
			const MatEval me = material_eval<TEX>(S, R.mat, sf.u, sf.v);   // renderer.cpp:458-463
			bool transparent = false;
			if constexpr (ALPHA) {
				if (!(me.opacity == 1.0f || fabsf(me.opacity - 1.0f) < kEps)) {   // renderer.cpp:466-472: the draw only matters when opacity != 1
					uint32_t px, py, sample;
					aov_sample_of(P, id, px, py, sample);
					transparent = draws(P, py * P.W + px, sample, 0u, pass, BLOCK_SURFACE).x > me.opacity;
				}
				if (transparent) {   // the same sample continues behind the surface: same depth, pass + 1 (shade_vertex)
					d = mk(in.dx[i], in.dy[i], in.dz[i]);
					o = sf.pos + d * kEps;
					d = normalize(d);
					pass++;
					through = pass <= 4096;   // shade_vertex's safety end; the sample then counts as a miss
				}
			}
			if (!transparent) {   // the sample's surface, back-facing or not (renderer.cpp:478 is the integrator's business)
				if constexpr (KIND == AOV_EMISSION) {
					// shade_vertex at depth 0: L = 0 + 1 * emissive10 unless the surface faces away (renderer.cpp:478-479). d is the direction
					// of the ray that found the surface, as the stream holds it
					const V3 nrm = shading_normal(sf, me.normal_ts), outcoming = -mk(in.dx[i], in.dy[i], in.dz[i]);
					if (dot(nrm, outcoming) > 0) ra = make_float4(me.emissive10.x, me.emissive10.y, me.emissive10.z, 1.0f);
				} else if constexpr (KIND == AOV_MOTION) {
					ra = motion_record(S, P, *Mo, surf, (uint32_t)H.triangle[i] + S.surfaces[surf].tri_base, H.b1[i], H.b2[i], sf.pos);
				} else {
					const V3 nrm = shading_normal(sf, me.normal_ts);   // intersect_result::get_normal()
					uint32_t cx, cy, csample;
					aov_sample_of(P, id, cx, cy, csample);
					V3 co;   // origin of THIS sample's camera ray: with a lens, its lens point; under motion, of the camera at the sample's time
					if (Rm && Rm->camera_moved) {
						DevScene Sc = S;
						camera_at(Sc, *Rm, u);
						co = camera_ray_origin(Sc, P, cx, cy, csample);
					} else co = camera_ray_origin(S, P, cx, cy, csample);
					ra = make_float4(me.albedo.x, me.albedo.y, me.albedo.z, 1.0f);
					rn = make_float4(nrm.x, nrm.y, nrm.z, length(sf.pos - co));
				}
			}
		}
		if (!through) {
			rec[id] = ra;
			if constexpr (KIND == AOV_GUIDES) rec[rec_stride + id] = rn;
		}
	}
	if constexpr (ALPHA) {
		// dense append: one atomic per wave reserves the wave's entries, the lane prefix count places them
		const uint64_t m = __ballot(through);
		if (m == 0) return;
		const int leader = __ffsll((long long)m) - 1;
		uint32_t base = 0;
		if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(n_out, (uint32_t)__popcll(m));
		base = __shfl(base, leader);
		if (through) {
			const uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));   // < n: a lane appends at most one entry
			out.ox[pos] = o.x; out.oy[pos] = o.y; out.oz[pos] = o.z;
			out.dx[pos] = d.x; out.dy[pos] = d.y; out.dz[pos] = d.z;
			out.id[pos] = id; out.pass[pos] = pass;
		}
	}
}

template <bool TEX, bool ALPHA>
__global__ void __launch_bounds__(kAovBlock) k_aov_shade(DevScene S, RenderParams P, AovStream in, AovHits H, uint32_t n, AovStream out, uint32_t* __restrict__ n_out,
                                                         float4* __restrict__ rec, size_t rec_stride, RenderMotion Rm) {
	aov_shade_sample<TEX, ALPHA, AOV_GUIDES>(S, P, in, H, n, out, n_out, rec, rec_stride, nullptr, &Rm);
}

template <bool TEX, bool ALPHA>
__global__ void __launch_bounds__(kAovBlock) k_aov_motion_shade(DevScene S, RenderParams P, AovStream in, AovHits H, uint32_t n, AovStream out, uint32_t* __restrict__ n_out,
                                                                float4* __restrict__ rec, AovMotion Mo) {
	aov_shade_sample<TEX, ALPHA, AOV_MOTION>(S, P, in, H, n, out, n_out, rec, 0, &Mo);
}

template <bool TEX, bool ALPHA>
__global__ void __launch_bounds__(kAovBlock) k_aov_emission_shade(DevScene S, RenderParams P, AovStream in, AovHits H, uint32_t n, AovStream out, uint32_t* __restrict__ n_out,
                                                                  float4* __restrict__ rec) {
	aov_shade_sample<TEX, ALPHA, AOV_EMISSION>(S, P, in, H, n, out, n_out, rec, 0, nullptr);
}

// Adds the pass's records of each pixel, in sample order, into the caller's buffers, as k_resolve does for radiance. A sample that ended on
// a miss (coverage 0) is skipped rather than added as zeros. Pixels outside a sharded pass's list are not touched.
__global__ void k_aov_resolve(const float4* __restrict__ rec, size_t rec_stride, float4* __restrict__ albedo_cov, float4* __restrict__ normal_depth,
                              const uint32_t* __restrict__ pixels, uint32_t n_pixels, uint32_t pass_spp) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n_pixels) return;
	const uint32_t dst = pixels ? pixels[p] : p;
	float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
	if (albedo_cov) a = albedo_cov[dst];
	if (normal_depth) b = normal_depth[dst];
	for (uint32_t s = 0; s < pass_spp; s++) {
		const size_t k = (size_t)s * n_pixels + p;
		const float4 ra = rec[k];
		if (ra.w == 0.f) continue;
		a.x += ra.x; a.y += ra.y; a.z += ra.z; a.w += ra.w;
		if (normal_depth) {
			const float4 rn = rec[rec_stride + k];
			b.x += rn.x; b.y += rn.y; b.z += rn.z; b.w += rn.w;
		}
	}
	if (albedo_cov) albedo_cov[dst] = a;
	if (normal_depth) normal_depth[dst] = b;
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_aov_generate(const DevScene& S, const RenderParams& P, const AovStream& out, uint32_t n, const RenderMotion& Rm, hipStream_t stream) {
	hipLaunchKernelGGL(k_aov_generate, dim3((n + kAovBlock - 1) / kAovBlock), dim3(kAovBlock), 0, stream, S, P, out, n, Rm);
	return hipGetLastError();
}

hipError_t launch_aov_shade(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* n_out, float4* rec,
                            size_t rec_stride, const RenderMotion& Rm, hipStream_t stream) {
	const dim3 grid((n + kAovBlock - 1) / kAovBlock), block(kAovBlock);
	if (S.any_texture) {
		if (S.any_alpha) hipLaunchKernelGGL((k_aov_shade<true, true>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, rec_stride, Rm);
		else hipLaunchKernelGGL((k_aov_shade<true, false>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, rec_stride, Rm);
	} else {
		if (S.any_alpha) hipLaunchKernelGGL((k_aov_shade<false, true>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, rec_stride, Rm);
		else hipLaunchKernelGGL((k_aov_shade<false, false>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, rec_stride, Rm);
	}
	return hipGetLastError();
}

hipError_t launch_aov_motion_shade(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* n_out, float4* rec,
                                   const AovMotion& Mo, hipStream_t stream) {
	const dim3 grid((n + kAovBlock - 1) / kAovBlock), block(kAovBlock);
	if (S.any_texture) {
		if (S.any_alpha) hipLaunchKernelGGL((k_aov_motion_shade<true, true>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, Mo);
		else hipLaunchKernelGGL((k_aov_motion_shade<true, false>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, Mo);
	} else {
		if (S.any_alpha) hipLaunchKernelGGL((k_aov_motion_shade<false, true>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, Mo);
		else hipLaunchKernelGGL((k_aov_motion_shade<false, false>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec, Mo);
	}
	return hipGetLastError();
}

hipError_t launch_aov_emission_shade(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* n_out, float4* rec,
                                     hipStream_t stream) {
	const dim3 grid((n + kAovBlock - 1) / kAovBlock), block(kAovBlock);
	if (S.any_texture) {
		if (S.any_alpha) hipLaunchKernelGGL((k_aov_emission_shade<true, true>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec);
		else hipLaunchKernelGGL((k_aov_emission_shade<true, false>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec);
	} else {
		if (S.any_alpha) hipLaunchKernelGGL((k_aov_emission_shade<false, true>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec);
		else hipLaunchKernelGGL((k_aov_emission_shade<false, false>), grid, block, 0, stream, S, P, in, H, n, out, n_out, rec);
	}
	return hipGetLastError();
}

hipError_t launch_aov_resolve(const float4* rec, size_t rec_stride, float4* albedo_cov, float4* normal_depth, const uint32_t* pixels, uint32_t n_pixels, uint32_t pass_spp,
                              hipStream_t stream) {
	hipLaunchKernelGGL(k_aov_resolve, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, rec, rec_stride, albedo_cov, normal_depth, pixels, n_pixels, pass_spp);
	return hipGetLastError();
}

}  // namespace ptx
