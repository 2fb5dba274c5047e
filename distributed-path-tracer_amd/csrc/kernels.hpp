// Kernel argument blocks and launchers shared by the .hip files and the C ABI (ptx_api.cpp, api_render.cpp, api_batch.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

#include "flat_scene.hpp"

namespace ptx {

#ifndef PTX_BLOCK
#define PTX_BLOCK 1024
#endif
constexpr int kBlock = PTX_BLOCK;  // threads per workgroup (one workgroup per CU): 1024 = 16 waves = 4 per SIMD
#ifndef PTX_CHUNK
#define PTX_CHUNK 2048
#endif
constexpr uint32_t kChunk = PTX_CHUNK; // camera paths a wave takes per counter fetch (32 wave-iterations). Measured with 64 spp per launch: 512 -7 %, 1024 0, 2048 +5.6 %, 4096 +6.3 % on Cornell; 4096 -12 % on the open plaza scene
// wave-private stream space, in float4
// Per-wave stream area in float4: 2 x 4 ray arrays + hit records (9 kChunk), hit distances (1/2), shadow requests (3), then one
// deferred list (2 x kListCap float4) per unit that can be set aside: per model, or per surface in the SURF kernels (<= 64 units:
// the list lengths live in the lanes of one VGPR).
#ifndef PTX_INLINE_MIN
#define PTX_INLINE_MIN 32
#endif
constexpr uint32_t kInlineMin = PTX_INLINE_MIN;        // lanes of a wave-iteration that make a unit worth traversing on the spot
constexpr uint32_t kListCap = (kChunk / 64u) * (kInlineMin - 1u) + 16u;   // entries a list can receive per chunk (kChunk / 64 iterations)
constexpr int kMaxDeferModels = 64;
constexpr uint32_t kQueueFixedFloat4 = 12u * kChunk + kChunk / 2u;
inline uint32_t queue_float4_per_wave(uint32_t n_units) { return kQueueFixedFloat4 + (n_units <= (uint32_t)kMaxDeferModels ? n_units : 0u) * 2u * kListCap; }
// the kernel addresses a wave's area with 32-bit byte offsets (device_core.hpp, Q4)
constexpr uint64_t kStreamAreaMaxBytes = ((uint64_t)kQueueFixedFloat4 + (uint64_t)kMaxDeferModels * 2u * kListCap) * 16u;
static_assert(kStreamAreaMaxBytes <= 0xFFFFFFFFull, "a wave's stream area must be addressable with a 32-bit byte offset");
constexpr uint32_t kSpillWords = 24u * 64u;  // uint2 per wave: kSpillStack levels x 64 lanes

// Device view of a FlatScene (all pointers are device pointers).
// Where a scene's KD nodes and triangle records live while a kernel runs (kernel template parameter MODE):
// everything in global memory (L2/HBM) | everything staged in LDS | hybrid: the surfaces that fit one CU's LDS
// (SurfaceRec::lds_root valid) staged, the large ones in global memory.
enum : int { MODE_GLOBAL = 0, MODE_LDS = 1, MODE_HYBRID = 2 };

struct DevScene {
	const ModelRec* models;
	const SurfaceRec* surfaces;
	const MaterialRec* materials;
	const uint2* nodes;      // KD nodes of all surfaces (global-memory traversal)
	const uint32_t* refs;    // unused by the kernels since the global path reads leaf-ordered records; kept for ptx_scene_get_array parity
	const float4* tris;   // 9 per triangle: the hit record (HitRec: corners + u, normals + v, tangents)
	// The triangle word that traversal records carry and hits report is `id | slot << 24` when tri_id_mask == 0x00FFFFFF (scenes of fewer
	// than 2^24 triangles): slot < n_hot = the triangle's hit record is also among the n_hot records of `hot_hitrec`, which the LDS kernels
	// stage into LDS (hot_lds, set inside the kernel) — the largest triangles, which take most hits; 0xFF = only in `tris`.
	const float4* hot_hitrec;
	const float4* hot_lds;
	uint32_t n_hot, tri_id_mask;
	const float4* tri_isect; // global-memory traversal: one TriIsect per leaf reference, in leaf order, triangle id in word 10; same allocation as `nodes`, behind them
	uint64_t geom_bytes;     // bytes of that allocation (nodes + records)
	// resident copy (staged into LDS by MODE_LDS / MODE_HYBRID kernels): nodes, refs and one TriIsect per triangle of the
	// surfaces that fit, indices rewritten to be local to these arrays (SurfaceRec::lds_root)
	const uint2* res_nodes;
	const uint32_t* res_refs;
	const float4* res_tris;
	uint32_t n_res_nodes, n_res_refs, n_res_tris;
	const ShadeRec* shade; // 1 per surface
	const SpaceRec* spaces; // distinct world->local transforms
	const TexRec* tex;       // textures
	const uint8_t* texels;   // 8-bit texel bytes of all textures
	const float* texels_f;   // float texels of Radiance .hdr images (TexRec::c_srgb & kTexFloat)
	const float* srgb_lut;   // [256] pow(b / 255, 2.2)
	uint32_t glb_leaf_ordered; // layout of tri_isect: 1 = one record per leaf reference (leaf order), 0 = one per triangle (reached through refs)
	uint32_t any_texture;
	int32_t env_tex;         // environment map (renderer::environment): texture index or -1
	const uint32_t* model_space; // per model
	const UnitAux* surf_aux;     // per surface: chain flag (flat_scene.hpp)
	const uint32_t* wf_order;    // [n_surfaces] queue-based pipeline: the surfaces in the order the traverse kernel starts their queues (upload_scene)
	int32_t n_models;
	uint32_t n_surfaces, n_nodes, n_refs, n_tris;
	uint32_t any_alpha;
	uint32_t n_spaces;
	CameraRec cam;
	SunRec sun;
	const float2* lens;      // [kLensMaxBlades + 1] the aperture's corners (ptx_scene_set_camera); read only where cam.lens_radius > 0
};

struct RenderParams {
	uint32_t W, H;              // full image
	uint32_t x0, y0, w, h;      // tile
	uint32_t n_pixels;          // w*h
	uint32_t sample0;           // first sample index of this pass
	uint32_t pass_spp;          // samples per pixel in this pass
	uint32_t bounces;
	uint32_t transparent;       // renderer::transparent_background (ptx_render_transparent): a sample that ends on a miss at depth 0 stores alpha 0
	                            // (k_wf_shade tests it; the fused kernel has a variant for it). Sits in what was padding: no other member moves
	uint64_t n_paths;           // n_pixels * pass_spp
	uint32_t seed_lo, seed_hi;
	float env[3];
	uint32_t integrator;        // ptx_integrator
	const uint32_t* pixels;     // nullptr: the pass covers every pixel of the tile; else [n_pixels] tile-local pixel indices (ly * w + lx)
	                            // of the pixels this pass renders (interleaved tile sharding), and n_pixels is the list's length
};

constexpr int kProfRegions = 28;   // PTX_PROF builds only: (wave-level trips, active lanes) per code region

struct PassBuffers {
	float4* queues;                   // [n_wave_slots][queue_stride]
	uint32_t queue_stride;            // float4 per wave: queue_float4_per_wave(units)
	uint32_t surface_units;           // 1: the SURF kernels (single surfaces are set aside), 0: whole models
	float4* sample_rad;               // [pass_spp][n_pixels]
	uint2* spill;                     // [n_wave_slots][kSpillWords]: traversal-stack overflow, lane-interleaved
	unsigned long long* chunk_counter; // paths handed out so far; zeroed before each pass
	unsigned long long* ray_counter;  // accumulates
};

// The motion table of a scene (ptx_scene_set_motion; one buffer the scene owns): the two keys of every model and which models move. A
// kernel argument of its own for the kernels that know time; DevScene does not carry it.
struct DevMotion {
	const float* begin_xform;   // [n_models][12] the state at u = 0 (origin, basis columns: PTX_ARR_MODEL_XFORM's layout)
	const float* end_xform;     // [n_models][12] the state at u = 1: the scene's current transforms
	const uint32_t* moved;      // [n_models] non-zero: the keys differ bitwise; the records of a model with 0 are the scene's own
};

// What the unfused integrators' kernels take about the scene's motion (k_nee_generate, k_nee_shade, k_aov_generate, k_aov_shade): a kernel
// argument of its own, as NeePunctual and AovMotion are. active == 0: no statement of motion runs (a wave-uniform test of this argument).
struct RenderMotion {
	DevMotion models;                     // read only where models_moved != 0
	float cam_begin[12];                  // the begin camera's origin and basis; read only where camera_moved != 0
	uint32_t active, camera_moved, models_moved;
	float shutter_open, shutter_close;
};
// time[i] = the time of the sample with id id[i] (id == nullptr: entry i is sample i): the times of a round's path stream, in stream order,
// as intersect_device's timed batch takes them (motion.hip)
hipError_t launch_motion_times(const RenderParams& P, const RenderMotion& Mo, const uint32_t* id, uint32_t n, float* time, hipStream_t stream);

struct IntersectArgs {
	const float *ox, *oy, *oz, *dx, *dy, *dz;
	size_t n;
	float* distance; int32_t* surface; int32_t* triangle;
	float *b0, *b1, *b2;
	float *px, *py, *pz, *nx, *ny, *nz, *u, *v;  // optional groups (nullptr = skip)
	uint2* spill;                                // [grid * waves per block][kSpillWords]
	const float* time;                           // nullptr: the scene at u = 1, the kernels that know no time; else [n] each ray's u (the motion kernels)
	DevMotion motion;                            // read only where time != nullptr
};

// Workspace of the queue-based pipeline (wavefront.hip). A PAIR is (ray, surface whose box it enters). Pair space is a POOL sized from
// demand (a ray enters 3-5 of an atrium's 24 surface boxes, not all of them): every classify tile (1024 rays) reserves its pairs with
// ONE atomic and uses its block of the pool twice — as queue entries grouped by surface (what the traversal waves read, contiguous
// per surface: one SEGMENT per tile and surface) and as result slots grouped by ray (what the shading / merge kernels read: the
// pairs of a ray are consecutive, in surface order). A step whose pairs do not fit the pool raises the overflow word; the host then
// repeats the slab in smaller pieces.
struct WfBuffers {
	float4* qent;                  // [pool_cap][2] queue entries: (local origin, result slot bits) (local direction, -)
	float4* pair_hit;              // [pool_cap] results: (local t, global triangle id bits, beta, gamma); t = -1: the walk found nothing
	uint32_t pool_cap;             // pairs the pool holds
	uint2* seg;                    // [n_surfaces][seg_cap]: (first entry, entries) of the segments of each surface's queue
	uint32_t seg_cap;              // classify tiles of a step at most
	uint32_t* first;               // [rays] first result slot of the ray
	unsigned long long* mask;      // [rays] bit u: the ray enters surface u
	uint32_t* ctl;                 // control block of THIS step (kWfCtlWords words, zeroed before the step; layout below)
	const uint32_t* n_in;          // device word: stream entries of this step (render) / rays of this slice (batch intersect)
	uint32_t* overflow;            // device word, sticky over the steps of a slab: some step's pairs did not fit the pool
	uint32_t* peak;                // device word: the most pairs any step of the slab asked for (what the host sizes the next slab by)
	uint2* spill;                  // [wf_traverse_grid * 4 waves][kSpillWords]
	unsigned long long* ray_counter;   // nullptr, or where classify adds the number of rays it was given (render statistics)
	uint32_t wave_clock;           // 1: every traverse wave that found work adds its run time to ctl[kWfCtlClock ..] (ptx_ctx_set_timing)
};
// control block of a step (uint32 words): [0] pairs reserved so far, [1] this step overflowed the pool, [kWfCtlSeg + u] segments of
// surface u's queue, [kWfCtlCur + 64 u] hand-out cursor of surface u's segments (256 bytes apart: two dozen hot counters in one
// cache line serialised every hand-out of the chip in one L2 channel), [kWfCtlProf ..] PTX_WF_PROF region counters
constexpr uint32_t kWfCtlSeg = 16, kWfCtlProf = 80, kWfCtlCur = 192, kWfCtlWords = kWfCtlCur + 64u * 64u;
constexpr uint32_t kWfCtlClock = kWfCtlProf + 72;   // [+0, +1] 64-bit sum of the working waves' run times (s_memtime ticks), [+2] such waves, [+3] the longest run
#ifndef PTX_WF_TILE
#define PTX_WF_TILE 1024
#endif
constexpr uint32_t kWfTile = PTX_WF_TILE;   // rays per classify tile = threads of a classify workgroup (measured: profiles/round3_wf_ab.txt)
// One of the two path-stream buffers of a render slab (SoA of float4, `cap` entries per array)
struct WfStream {
	float4* q;   // [4][cap]: (origin, id | flags) (direction, T.x) (T.y, T.z, L.x, L.y) (L.z, depth << 16 | pass, RNG key pixel, RNG key sample) — the fused kernel's entry
	float4* r;   // [3][cap]: the entry's shadow request: (origin, -) (direction, -) (x: radiance to add when unoccluded | origin of a shadow catcher's pass-through ray, -)
};
// flags in the id word of a stream entry (ids are slab-local, < 2^28)
constexpr uint32_t kWfIdMask = 0x0FFFFFFFu, kWfZombie = 1u << 31, kWfPending = 1u << 30, kWfRequest = 1u << 29;
constexpr uint32_t kWfMaxSlab = 1u << 27;   // paths of a slab at most: the whole 128 Mi-path pass (the stream buffers of a slab take 224 bytes per path; ids have 28 bits)
constexpr int kWfMaxSurfaces = 64;   // surface masks are one 64-bit word
// persistent 256-thread workgroups of the traverse kernel: as many as can be resident (59 VGPRs and 24 KB of LDS allow 6 per CU; 8 are launched)
inline int wf_traverse_grid(int n_cu) { return n_cu * 8; }
// a slab's steps run back to back on the device: step s reads its entry count from flow[s] and adds what it emits to flow[s + 1]
hipError_t launch_wf_generate(const DevScene& S, const RenderParams& P, const WfStream& out, uint32_t cap, uint32_t first, uint32_t n, float4* sample_rad, hipStream_t stream);
hipError_t launch_wf_step(const DevScene& S, const RenderParams& P, const WfBuffers& W, const WfStream& in, const WfStream& out, uint32_t cap, uint32_t max_in,
                          uint32_t slab_first, uint32_t* n_out, float4* sample_rad, int n_cu, hipStream_t stream, hipEvent_t* ev /* nullptr, or 4 events: before classify / traverse / shade, after */);
hipError_t launch_wf_intersect(const DevScene& S, const IntersectArgs& A, size_t first_ray, uint32_t n, const WfBuffers& W, int n_cu, hipStream_t stream);

hipError_t launch_render_pass(const DevScene& S, const RenderParams& P, const PassBuffers& B, int mode, size_t lds_bytes, int grid,
                              hipStream_t stream);
hipError_t launch_resolve(const float4* sample_rad, float4* accum, const uint32_t* pixels, uint32_t n_pixels, uint32_t pass_spp, hipStream_t stream);
// the pass's samples s < n_a (<= pass_spp) of each pixel into accum_a, the rest into accum_b, each as launch_resolve adds them
hipError_t launch_resolve_halves(const float4* sample_rad, float4* accum_a, float4* accum_b, const uint32_t* pixels, uint32_t n_pixels, uint32_t pass_spp, uint32_t n_a,
                                 hipStream_t stream);
hipError_t launch_resolve_claim(const float4* sample_rad, float4* pixel_rgba, uint8_t* claimed, const uint32_t* pixels, uint32_t n_pixels, uint32_t pass_spp,
                                uint32_t sample0 /* global index of the pass's first sample */, hipStream_t stream);
hipError_t launch_intersect(const DevScene& S, const IntersectArgs& A, int mode, size_t lds_bytes, int grid, hipStream_t stream);
// the same batch with a time per ray (A.time and A.motion set; motion.hip): k_intersect_batch_motion
hipError_t launch_intersect_motion(const DevScene& S, const IntersectArgs& A, int mode, size_t lds_bytes, int grid, hipStream_t stream);
hipError_t launch_pbr_eval(const float* in, float* out, size_t n, hipStream_t stream);
constexpr uint32_t kLeafBatchMaxTris = 256;   // k_leaf_intersect: triangles of its one leaf at most (48 bytes each in LDS)
// `spill`: [grid * 4 waves][kSpillWords]; grid workgroups of 256 threads
hipError_t launch_leaf_intersect(const uint2* nodes, const uint32_t* refs /* [n_tri] */, const float4* tris /* [n_tri][3] */, uint32_t n_tri, uint32_t leaf_ordered /* 0 refs + LDS, 1 leaf order in global memory, 2 leaf order in LDS */,
                                 const float* rays /* [n][7] */, size_t n, float* out /* [n][3] */, int32_t* tri /* [n] */, uint2* spill, int grid, hipStream_t stream);
constexpr uint32_t kExactMathForms = 3;   // k_exact_math_check: one counter per form
hipError_t launch_exact_math_check(unsigned long long* bad /* [kExactMathForms], device, zeroed */, hipStream_t stream);
hipError_t launch_shade_consts_check(const float* in /* [n][9] */, const ShadeRec* rec /* [n] */, size_t n, unsigned long long* bad /* device, zeroed */, hipStream_t stream);
hipError_t launch_camera_rays(const DevScene& S, const float* in /* [n][3]: ndc.x ndc.y ratio */, float* out /* [n][6] */, size_t n, hipStream_t stream);
hipError_t launch_camera_lens_rays(const DevScene& S, const float* in /* [n][5]: ndc.x ndc.y ratio u v */, float* out /* [n][6] */, size_t n, hipStream_t stream);
hipError_t launch_material_eval(const DevScene& S, const int32_t* surface /* [n] */, const float* uv /* [n][2] */, size_t n, float* out /* [n][12] */, hipStream_t stream);
hipError_t launch_tonemap(const float4* accum, uint32_t n_pixels, float spp, const float* thresholds /* [256], device */, uchar4* out, hipStream_t stream);

// First-hit guide buffers (aov.hip, ptx_render_aov). A ROUND = the live samples' rays through the scene's own intersect route, then one
// k_aov_shade lane per sample: it either records the sample's surface or appends the ray behind an opacity pass-through to the next
// round's stream. Rays are SoA of floats — the layout both intersect launches read (IntersectArgs).
struct AovStream {
	float *ox, *oy, *oz, *dx, *dy, *dz;   // [cap]
	uint32_t* id;     // [cap] the sample's id within the pass (sample-major, pixel-minor); nullptr = entry i is sample i, pass 0 (round 0)
	uint32_t* pass;   // [cap] pass-throughs behind the sample so far
};
struct AovHits {   // what the intersect launch wrote for the round's rays
	const int32_t *surface, *triangle;   // -1 = miss; triangle index within the surface's mesh
	const float *b1, *b2;
};
hipError_t launch_aov_generate(const DevScene& S, const RenderParams& P, const AovStream& out, uint32_t n, const RenderMotion& Rm, hipStream_t stream);
// rec: [2][rec_stride] per-sample records of the pass, indexed by sample id: (albedo, 1) and (shading normal, depth); zeros for a sample that
// ends on a miss. *n_out (device, zeroed before the launch) receives the number of entries appended to `out`; untouched when the scene has
// no pass-through material (DevScene::any_alpha == 0)
// Rm: the scene's motion (active == 0: none); the guide kernels alone take it: ptx_render_motion and ptx_render_emission refuse active motion
hipError_t launch_aov_shade(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* n_out,
                            float4* rec, size_t rec_stride, const RenderMotion& Rm, hipStream_t stream);
// ptx_render_motion: the previous frame as k_aov_motion_shade takes it. The camera travels in the kernel argument; the transforms live in
// context workspace.
struct AovMotion {
	float origin[3], basis[9], tan_half_fov;   // the previous camera (the current one when it did not move); a lens is ignored
	const float* prev_xform;                   // [n_models][12] (origin, basis columns: PTX_ARR_MODEL_XFORM), or nullptr: no model moved
	const uint32_t* moved;                     // [n_models] non-zero: the model's previous transform differs bitwise from its current one
};
// the same walk as launch_aov_shade; rec: [rec_stride] ONE record per sample, (previous - current pixel position, distance from the previous
// camera, 1), zeros for a sample that contributes nothing. launch_aov_resolve(rec, ..., motion, nullptr, ...) adds them up.
hipError_t launch_aov_motion_shade(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* n_out, float4* rec,
                                   const AovMotion& Mo, hipStream_t stream);
// ptx_render_emission: the same walk again; rec: [rec_stride] ONE record per sample, (emissive10, 1) of a surface that faces the ray that
// found it, zeros for a back-facing surface and for a miss. launch_aov_resolve(rec, ..., emission, nullptr, ...) adds them up.
hipError_t launch_aov_emission_shade(const DevScene& S, const RenderParams& P, const AovStream& in, const AovHits& H, uint32_t n, const AovStream& out, uint32_t* n_out, float4* rec,
                                     hipStream_t stream);
// adds the pass's records of each pixel, in sample order, into the caller's buffers (either may be nullptr)
hipError_t launch_aov_resolve(const float4* rec, size_t rec_stride, float4* albedo_cov, float4* normal_depth, const uint32_t* pixels, uint32_t n_pixels, uint32_t pass_spp,
                              hipStream_t stream);

// Next-event estimation towards emissive triangles (nee.hip, ptx_render_nee). A ROUND = the live paths' rays through the scene's own intersect
// route, k_nee_shade (one path vertex per lane), the round's shadow rays through the same route, k_nee_settle (their answers).
struct NeeStream {   // path state, SoA, `cap` entries per array; the six ray arrays are what the intersect launches read
	float *ox, *oy, *oz, *dx, *dy, *dz;
	float *tx, *ty, *tz;   // throughput
	float* pp;             // max(pdf, eps) of the direction sampled at the previous vertex
	uint32_t* id;          // the sample's id within the pass (sample-major, pixel-minor)
	uint32_t* dp;          // depth << 16 | pass
};
// x_prev of a stream's entries, the position of the vertex that drew the BSDF sample: three arrays beside a NeeStream's, allocated, written
// and read in tree mode only (PTX_LIGHT_PICK_TREE; else all nullptr). A struct of its own, the kernels' last argument, so that the
// arguments of the kernels that never read it stay where they were.
struct NeePrev {
	float *px, *py, *pz;
};
struct NeeHits {   // what an intersect launch wrote
	const float* distance;
	const int32_t *surface, *triangle;   // -1 = miss; triangle index within the surface's mesh
	const float *b1, *b2;
};
constexpr uint32_t kNeeNone = 0x7FFFFFFFu, kNeeCatcher = 0x80000000u;   // sun_pos / light_pos: no such ray | the sun ray is a shadow catcher's
struct NeeShadow {
	float *ox, *oy, *oz, *dx, *dy, *dz;   // [2 cap] the round's shadow rays, dense
	float *sx, *sy, *sz;                  // [cap] by path: radiance the sun adds when unoccluded | origin of a lit catcher's pass-through ray
	float *lx, *ly, *lz;                  // [cap] by path: radiance the light sample adds when visible
	uint32_t *sun_pos, *light_pos;        // [cap] by path: the ray's position in the shadow stream (< 2^31), or kNeeNone
	uint32_t *exp_surf, *exp_tri;         // [cap] by path: the sampled triangle (surface, local triangle)
	float* tm;                            // [2 cap] the time of each shadow ray, beside it; written and read under active motion only (else nullptr)
};
struct NeeLights {   // the scene's light list (ptx_api.cpp: build_lights); n == 0: no light samples, every emission weight is 1
	const uint2* tris;           // [n] (surface, local triangle), ordered by surface, then triangle
	const float* cdf;            // [n] cumulative area share, the last entry 1
	const float4* geom;          // [n] geometric normal (world), area
	const int32_t* surf_first;   // [n_surfaces] first entry of the surface, or -1
	uint32_t n;
	float area;                  // A_total
	// The light tree of PTX_LIGHT_PICK_TREE (ptx_api.cpp: build_light_tree). nodes == nullptr: CDF mode. A node is two float4:
	// (lo.xyz, power) (hi.xyz, word 7), word 7 = 0x80000000 | entry for a leaf, else the left child's index; the right child is the next node.
	const float4* nodes;
	const uint32_t* path;        // [n] bit i = step i of the descent to the entry's leaf goes right
	uint32_t n_nodes;
};
// the stochastic pick alone, one (position, u) per lane (ptx_light_pick_batch), and the directed pmf of a given entry, one (position, entry)
// per lane (ptx_light_pmf_batch): the device functions nee_candidate and nee_vertex inline
hipError_t launch_light_pick(const NeeLights& Lt, const float* pos_u /* [n][4] */, size_t n, int32_t* light, float* pmf, hipStream_t stream);
hipError_t launch_light_pmf(const NeeLights& Lt, const float* pos /* [n][3] */, const int32_t* light, size_t n, float* pmf, hipStream_t stream);
// The environment map's sampling table (ptx_api.cpp: build_env_table), PTX_NEE_ENV_SAMPLES. row_cdf == nullptr: no table, the unflagged estimator
struct NeeEnv {
	const float* row_cdf;    // [h] cumulative share of the rows' mass, top row first, the last entry 1
	const float* cell_cdf;   // [h][w] cumulative share of the boxes within their row, the last entry 1 (a row of zero mass: all 0)
	uint32_t w, h;           // the map's size in texels
};
constexpr uint32_t kNeeEnvRay = 0xFFFFFFFFu;   // exp_surf of an environment sample's shadow ray: the sample is visible iff the ray hits nothing
// The scene's punctual lights (ptx_scene_set_punctual_lights). n == 0: none, and the kernels without the punctual branch run. The variants
// with the branch (template parameter PUN) are the only readers: every other kernel takes no argument of this kind.
struct NeePunctual {
	const float4* recs;   // [n][4] the 16-float records as stored: (position, range) (direction, kind) (intensity, cos_inner) (cos_outer, 0, 0, 0)
	const float* cdf;     // [n] cumulative share of lum(intensity), the last entry 1
	uint32_t n;
	// The light tree of PTX_PUNCTUAL_PICK_TREE (ptx_api.cpp: build_punctual_tree). nodes == nullptr: the pick is the CDF's. A node is two float4:
	// (lo.xyz, power) (hi.xyz, word 7), word 7 = 0x80000000 | light for a leaf, else the left child's index; the right child is the next node.
	const float4* nodes;
	uint32_t n_nodes;
};
// the pick alone, one (position, u) per lane (ptx_punctual_pick_batch): the device function nee_candidate inlines
hipError_t launch_punctual_pick(const NeePunctual& Pn, const float* pos_u /* [n][4] */, size_t n, int32_t* light, float* pmf, hipStream_t stream);
constexpr uint32_t kNeePunctualRay = 0xFFFFFFFEu;   // exp_surf of a punctual sample's shadow ray: exp_tri holds the bits of dist, and the sample is visible iff the ray hits nothing nearer than dist
// cnt (device, 8 words): [0] entries appended to `out`, [1] shadow rays of the round, [2..3] light samples (64-bit), [4..5] visible ones
hipError_t launch_nee_generate(const DevScene& S, const RenderParams& P, const NeeStream& out, float4* L, uint32_t n, const RenderMotion& Mo, hipStream_t stream);
// sampler_pdf: the variants of PTX_NEE_SAMPLER_PDF (nee_core.hpp: sampler_pdf in pe's place in the weights)
// candidates: M of PTX_NEE_CANDIDATES, 1 .. 16; above 1 the RIS variants run (nee_core.hpp: the candidate loop of nee_vertex)
// Pn.n != 0: the PUN variants run (part 1 of nee.hip), and launch_nee_settle is told so: its punctual form knows kNeePunctualRay
hipError_t launch_nee_shade(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates, const NeeStream& in,
                            const NeeHits& H, uint32_t n, const NeeStream& out, const NeeShadow& W, uint32_t* cnt, float4* L, const RenderMotion& Mo, const NeePrev& in_prev, const NeePrev& out_prev,
                            hipStream_t stream);
hipError_t launch_nee_settle(const NeeStream& in, uint32_t n, const NeeShadow& W, const NeeHits& SH, const NeeStream& out, uint32_t* cnt, float4* L, bool punctual, const NeePrev& in_prev, const NeePrev& out_prev, hipStream_t stream);   // in_prev.px != nullptr: tree mode

// The same estimator in one launch per pass (nee_fused.hip, PTX_NEE_FUSED): persistent workgroups as launch_render_pass sizes them, a lane per path,
// no streams. The only per-sample memory is sample_rad.
struct NeeFusedBuffers {
	float4* sample_rad;                  // [pass_spp][n_pixels]: (L, 1) of every sample of the pass
	uint2* spill;                        // [grid * kBlock / 64][kSpillWords]: traversal-stack overflow, lane-interleaved
	unsigned long long* chunk_counter;   // paths handed out so far; zeroed before each pass
	unsigned long long* counters;        // [3] accumulate: rays (closest + both shadow kinds), light samples, visible light samples
};
hipError_t launch_nee_fused(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates,
                            const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream);
// The fused kernel with a time per lane (nee_fused_motion.hip, PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION under active motion): Mo as launch_nee_shade
// takes it. Mo.active == 0, or models_moved without the motion table, is hipErrorInvalidValue: never a static launch.
hipError_t launch_nee_fused_motion(const DevScene& S, const RenderParams& P, const NeeLights& Lt, const NeeEnv& Ev, const NeePunctual& Pn, bool sampler_pdf, uint32_t candidates,
                                   const RenderMotion& Mo, const NeeFusedBuffers& B, int mode, size_t lds_bytes, int grid, hipStream_t stream);

// Variance-guided a-trous filter (denoise.hip, ptx_denoise). All buffers [n_pixels] float4 on the device.
// prepare: the two radiance sums and the guide sums -> col_var (demodulated colour, v0), guide (mean normal, mean depth), remod (albedo, alpha)
hipError_t launch_denoise_prepare(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, uint32_t spp_a, uint32_t spp_b, size_t n_pixels,
                                  float4* col_var, float4* guide, float4* remod, hipStream_t stream);
// the same with per-pixel sample counts: a.w and b.w are the halves' counts, the guides hold guide_spp samples of every pixel (ptx_denoise_counts)
hipError_t launch_denoise_prepare_counts(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, uint32_t guide_spp, size_t n_pixels,
                                         float4* col_var, float4* guide, float4* remod, hipStream_t stream);
// 3 x 3 variance prefilter: in (col, v0) -> out (col, var)
hipError_t launch_denoise_prefilter(const float4* in, const float4* guide, uint32_t W, uint32_t H, float sigma_n, float sigma_z, float4* out, hipStream_t stream);
// one iteration at `step`: in (col, var) -> out (col, var), or, with `last`, out = (col * albedo, alpha) of remod. tiled: the LDS-staged form
// (same arithmetic in the same order). `out` must not be `in`.
hipError_t launch_denoise_atrous(const float4* in, const float4* guide, const float4* remod, uint32_t W, uint32_t H, uint32_t step, float sigma_l, float sigma_n, float sigma_z,
                                 bool last, bool tiled, float4* out, hipStream_t stream);

// Temporal accumulation in front of the filter (temporal.hip, ptx_denoise_temporal): k_tp_accumulate in k_dn_prepare's place.
struct TemporalHistory {   // [n_pixels] each, device; all nullptr: no history (the first frame)
	float4* color;      // integrated demodulated colour, history length
	float2* moments;    // integrated first and second moment of the luminance
	float4* geometry;   // mean normal, mean depth
};
struct TemporalParams {
	int W, H;
	float n, na, nb;   // float(spp_a + spp_b), float(spp_a), float(spp_b)
	float max_history, tau_z, tau_n;
};
// The two pixel counts of a launch are spread over kTpCounterSlots words, kTpCounterStride words apart (a cache line each): every wave adds
// to the slot of its workgroup with one atomic. With ONE word for the 32 400 waves of a 1080p frame the kernel took 0.40 ms on the MI355X, with
// the slots 0.075 ms. The host adds the slots up.
constexpr uint32_t kTpCounterSlots = 128, kTpCounterStride = 16;
constexpr size_t kTpCounterBytes = (size_t)kTpCounterSlots * kTpCounterStride * sizeof(unsigned long long);
// col_var == nullptr: only the history is advanced (guide and remod are not written either). counter (device, kTpCounterBytes, zeroed before
// the launch): each slot receives pixels that took history in its low 32 bits and pixels that started over in its high 32.
hipError_t launch_temporal_accumulate(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, const float4* motion, const TemporalHistory& prev,
                                      const TemporalHistory& next, const TemporalParams& T, float4* col_var, float4* guide, float4* remod, unsigned long long* counter,
                                      hipStream_t stream);
// The same kernel for half-buffers with per-pixel sample counts in .w (ptx_denoise_temporal_counts): T.n = float(guide_spp), T.na and T.nb
// are not read, T.max_history and the history length count samples. search, unit_normals: PTX_TEMPORAL_SEARCH_3X3, PTX_TEMPORAL_UNIT_NORMALS.
hipError_t launch_temporal_accumulate_counts(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, const float4* motion,
                                             const TemporalHistory& prev, const TemporalHistory& next, const TemporalParams& T, bool search, bool unit_normals, float4* col_var,
                                             float4* guide, float4* remod, unsigned long long* counter, hipStream_t stream);

// Noise-driven per-pixel sample counts (adaptive.hip; ptx_render_adaptive, ptx_adaptive_select, ptx_accum_mean). A TILE is 32 x 32 pixels of the
// rectangle, anchored at its origin (one workgroup), a BLOCK 8 x 8 (one wave-iteration): 16 blocks per tile, row-major.
constexpr uint32_t kAdTile = 32, kAdBlocksPerTile = 16, kAdMaxSide = 16384;   // 2^18 tiles at most: one workgroup scans their counts
struct AdaptiveBuffers {   // device workspace of one decision on a w x h rectangle
	uint8_t* noisy;                  // [w * h] 1 = the two halves disagree by more than the threshold
	unsigned long long* block_mask;  // [tiles][16] active lanes of the block (lane = ry * 8 + rx)
	uint32_t* block_off;             // [tiles][16] active pixels of the tile before the block
	uint32_t* tile_count;            // [tiles]
	uint32_t* tile_off;              // [tiles] active pixels before the tile
	uint32_t* n_active;              // one word: the list's length
};
// one decision: a, b [w * h] radiance sums; `done` [w * h] in/out; `pixels` [w * h] receives the active list (nullptr: none is written)
hipError_t launch_adaptive_select(const float4* a, const float4* b, uint32_t w, uint32_t h, float threshold, const AdaptiveBuffers& B, uint8_t* done, uint32_t* pixels,
                                  hipStream_t stream);
// Interleaved tile sharding of a decision (ptx_ctx_set_mask_exchange): the rectangle's origin in the image, the shard tile's side, the shard
// tiles per image row and the rank. A pixel (x, y) of the image is the rank's own when ((y / ts) * tiles_x + x / ts) % count == index; the
// caller has checked that the image's tile indices fit 32 bits.
struct AdaptiveShard {
	uint32_t x0, y0, ts, tiles_x, index, count;
};
// the noisy bytes of the rank's own pixels, 0 for the others -> mask [w * h]
hipError_t launch_adaptive_noisy_shard(const float4* a, const float4* b, uint32_t w, uint32_t h, float threshold, const AdaptiveShard& shard, uint8_t* mask, hipStream_t stream);
// the decision of the whole rectangle from the merged mask (nonzero = noisy): `done` for every pixel, `pixels` the rank's own active pixels in
// list order; B.n_active receives two words, the own count and the count of all active pixels. tile_count_all: [tiles] scratch.
hipError_t launch_adaptive_decide_shard(const uint8_t* merged, uint32_t w, uint32_t h, const AdaptiveShard& shard, const AdaptiveBuffers& B, uint32_t* tile_count_all, uint8_t* done,
                                        uint32_t* pixels, hipStream_t stream);
// out = (a + b) / (a.w + b.w) for all four channels, or a / a.w when b == nullptr; out may be a or b
hipError_t launch_accum_mean(const float4* a, const float4* b, size_t n_pixels, float4* out, hipStream_t stream);

// First-hit emission around the filters (emission.hip; ptx_emission_split, ptx_emission_merge). e = emission.rgb / float(guide_spp); a
// channel whose e is not > 0 is left without arithmetic; .w of every buffer is untouched.
// a.c -= a.w * e.c, and the same for b unless it is nullptr; in place
hipError_t launch_emission_split(const float4* emission, uint32_t guide_spp, size_t n_pixels, float4* a, float4* b, hipStream_t stream);
// out.c += e.c; in place
hipError_t launch_emission_merge(const float4* emission, uint32_t guide_spp, size_t n_pixels, float4* out, hipStream_t stream);

}  // namespace ptx
