// Motion blur, fused route: closest hits of a batch of rays that each carry a time u in [0, 1] (include/ptx.h: MOTION). The scene as it
// stands is the state at u = 1, the scene's motion table (kernels.hpp: DevMotion) holds the state at u = 0. k_intersect_batch_motion is
// k_intersect_batch with scene_traverse_motion in scene_traverse's place: static ray spaces are transformed into from the scalar-loaded
// SpaceRec as ever, and for a moving space every lane blends the two keys at its own u and inverts the result itself, with the function
// the scene builder uses (flat_scene.hpp: derive_xform), so that a ray of time u sees bit for bit the scene set to the transforms at u.
// The KD trees are mesh-local: the walks (device_core.hpp) do not know about time.
//
// A translation unit of its own: kernels.hip and its pass code are not touched by motion.
#include "device_core.hpp"

namespace ptx {

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_intersect_batch_motion(DevScene S0, IntersectArgs A0, const ModelRec* __restrict__ t_models, const SurfaceRec* __restrict__ t_surfaces,
                                                                  const SpaceRec* __restrict__ t_spaces, const uint32_t* __restrict__ t_model_space,
                                                                  const UnitAux* __restrict__ t_surf_aux, const float* __restrict__ t_begin, const float* __restrict__ t_end,
                                                                  const uint32_t* __restrict__ t_moved) {
	DevScene S = S0;
	S.models = t_models; S.surfaces = t_surfaces; S.spaces = t_spaces; S.model_space = t_model_space; S.surf_aux = t_surf_aux;  // see struct Tables
	IntersectArgs A = A0;
	A.motion.begin_xform = t_begin; A.motion.end_xform = t_end; A.motion.moved = t_moved;   // scalar-loaded like the tables: the model index is wave-uniform
	const Staged st = stage_geometry<MODE>(S, g_smem);
	S.hot_lds = st.hot;
	const Geoms g = st.g;
	const Spill spill{A.spill + (size_t)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * (kSpillStack * 64) + (threadIdx.x & 63u)};
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += stride) {
		const V3 o = mk(A.ox[i], A.oy[i], A.oz[i]), d = mk(A.dx[i], A.dy[i], A.dz[i]);
		const float u = A.time[i];
		SceneHit h;
		const bool hit = scene_traverse_motion<MODE>(S, A.motion, g, o, d, u, h, spill);
		write_hit_outputs_motion(S, st.shade, A, i, hit, h, u);
	}
}

template <int MODE>
static hipError_t launch_intersect_motion_mode(const DevScene& S, const IntersectArgs& A, size_t lds_bytes, int grid, hipStream_t stream) {
	if (MODE != MODE_GLOBAL) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_intersect_batch_motion<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_intersect_batch_motion<MODE>, dim3(grid), dim3(kBlock), MODE != MODE_GLOBAL ? lds_bytes : 0, stream, S, A, S.models, S.surfaces, S.spaces, S.model_space,
	                   S.surf_aux, A.motion.begin_xform, A.motion.end_xform, A.motion.moved);
	return hipGetLastError();
}
hipError_t launch_intersect_motion(const DevScene& S, const IntersectArgs& A, int mode, size_t lds_bytes, int grid, hipStream_t stream) {
	if (!A.time || !A.motion.begin_xform || !A.motion.end_xform || !A.motion.moved) return hipErrorInvalidValue;   // a missing table is an error, never a static launch
	if (mode == MODE_LDS) return launch_intersect_motion_mode<MODE_LDS>(S, A, lds_bytes, grid, stream);
	if (mode == MODE_HYBRID) return launch_intersect_motion_mode<MODE_HYBRID>(S, A, lds_bytes, grid, stream);
	return launch_intersect_motion_mode<MODE_GLOBAL>(S, A, lds_bytes, grid, stream);
}

// The times of a round's rays in stream order: entry i belongs to the sample with id id[i] (nullptr: entry i is sample i), whose time is a
// function of its pixel and sample index (sample_time). Sample ids are sample-major, pixel-minor within the pass, as nee.hip's and
// aov.hip's are.
__global__ void __launch_bounds__(256) k_motion_times(RenderParams P, RenderMotion Mo, const uint32_t* __restrict__ id, uint32_t n, float* __restrict__ time) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = id ? id[i] : i;
	const uint32_t s_local = s / P.n_pixels, p = s - s_local * P.n_pixels;
	const uint32_t local = P.pixels ? P.pixels[p] : p;
	const uint32_t px = P.x0 + local % P.w, py = P.y0 + local / P.w;
	time[i] = sample_time(P, Mo, py * P.W + px, P.sample0 + s_local);
}
hipError_t launch_motion_times(const RenderParams& P, const RenderMotion& Mo, const uint32_t* id, uint32_t n, float* time, hipStream_t stream) {
	hipLaunchKernelGGL(k_motion_times, dim3((n + 255u) / 256u), dim3(256), 0, stream, P, Mo, id, n, time);
	return hipGetLastError();
}

}  // namespace ptx
