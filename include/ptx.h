/* ptx.h — C ABI of the MI355X-native path-tracing integrator (libptx_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of vmanam0451/distributed-path-tracer: the
 * ray-intersection + Monte-Carlo shading integrator of path-tracer-core/path_tracer_lib.
 * The reference has no FFI layer (the host links the library statically and calls C++ classes,
 * path-tracer-core/CMakeLists.txt:44); each entry point below names the reference interface it
 * replaces. Paths are relative to path-tracer-core/; LIB = path_tracer_lib/path_tracer.
 *
 * Conventions: plain pointers and sizes only; every function returns a ptx_status (0 = ok) and never
 * throws; ptx_last_error() gives the thread-local message of the last failure. Buffers that the
 * documentation marks "device or host" may be either: the library inspects the pointer
 * (hipPointerGetAttributes) and stages host buffers through its own device workspace.
 * A scene is immutable after creation; one context per GPU; calls on one context are serialised
 * on that context's HIP stream.
 */
#ifndef PTX_H
#define PTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ptx_status {
	PTX_OK = 0,
	PTX_ERR_INVALID = 1,    /* bad argument */
	PTX_ERR_IO = 2,         /* file could not be read (LIB/core/renderer.cpp:64-69 only logs this and then crashes) */
	PTX_ERR_PARSE = 3,      /* malformed glTF */
	PTX_ERR_NO_CAMERA = 4,  /* "Scene does not contain camera #i." / "Scene is missing a camera." renderer.cpp:73-74,97-98 */
	PTX_ERR_NO_DEVICE = 5,  /* no HIP device / host-only scene used for GPU work: the product never falls back to a CPU path */
	PTX_ERR_HIP = 6,        /* HIP runtime error (message carries hipGetErrorString) */
	PTX_ERR_UNSUPPORTED = 7 /* feature outside the built scope (e.g. non-PNG or interlaced textures), refused rather than rendered wrong */
} ptx_status;

typedef struct ptx_ctx ptx_ctx;     /* one per GPU: device, stream, workspace */
typedef struct ptx_scene ptx_scene; /* flattened, immutable scene (+ its device copy) */

const char* ptx_last_error(void);
const char* ptx_version(void);

/* ---- context ------------------------------------------------------------------------------------
 * device >= 0: HIP device ordinal. Fails with PTX_ERR_NO_DEVICE when there is none. */
int ptx_ctx_create(int device, ptx_ctx** out);
/* Scenes created on the context keep it alive: it is freed together with the last of them, in whatever order the handles
 * are destroyed. */
void ptx_ctx_destroy(ptx_ctx* ctx);
/* Stream the context launches on (hipStream_t as void*), for callers that time or order work. */
void* ptx_ctx_stream(ptx_ctx* ctx);
int ptx_ctx_synchronize(ptx_ctx* ctx);

/* ---- scene load ---------------------------------------------------------------------------------
 * Replaces core::renderer::load_gltf(path) (LIB/core/renderer.hpp:35, renderer.cpp:61-331) and the
 * host's cloud::distributed_scene::load_scene (src/scene/scene.hpp:19): parses the glTF, builds the
 * entity transforms, unpacks every primitive (with the reference's loader quirks), builds one SAH
 * KD-tree per primitive with the reference's topology (LIB/core/mesh.cpp:131-298) and flattens all of
 * it into pointer-free arrays. ctx may be NULL: the scene is then host-only (inspection, no GPU work). */
typedef struct ptx_work_item {   /* one entry of models::work_info::work (src/models/work_info.hpp:11-15) */
	const char* mesh_name;
	const int32_t* primitives;
	uint32_t n_primitives;
} ptx_work_item;
typedef struct ptx_load_opts {
	uint32_t camera_index;    /* renderer.hpp:31, default 0 */
	uint32_t sun_light_index; /* renderer.hpp:32, default 0; 0xFFFFFFFF = renderer::no_sun_light */
	/* The host's per-worker primitive filter (distributed_scene::load_scene's scene_work, src/scene/load_gltf.cpp:93-99):
	 * when filter_primitives != 0 only the listed primitive indices of each named mesh are loaded, and a mesh that is not
	 * listed loads none (its model stays, empty). 0 = load everything, as core::renderer::load_gltf does. */
	uint32_t filter_primitives;
	uint32_t n_work;
	const ptx_work_item* work;
} ptx_load_opts;
int ptx_scene_load_gltf(ptx_ctx* ctx, const char* gltf_path, const ptx_load_opts* opts /* NULL = defaults */,
                        ptx_scene** out);

/* The reference worker's entry: a Lambda event (models::worker_info, src/models/work_info.hpp:17-32; sample in
 * path-tracer-core/events/event.json) names the scene, this worker's primitives, samples, bounces and X x Y
 * (src/main.cpp:9-25 -> processors::worker::run, worker.cpp:25-38). S3 is out of scope: `local_scene_root` is a local
 * directory holding the event's scene_root files; `<local_scene_root>/scene.gltf` is loaded with the event's filter.
 * cfg receives W, H, spp, bounces (+ defaults for the rest), ready for ptx_render. info may be NULL. */
typedef struct ptx_worker_event {
	int32_t num_workers;
	uint32_t n_work_meshes;
	char worker_id[64];
	char scene_root[256];
	char scene_bucket[128];
} ptx_worker_event;
struct ptx_render_cfg;
int ptx_worker_event_load(ptx_ctx* ctx, const char* event_json_path, const char* local_scene_root, ptx_scene** scene,
                          struct ptx_render_cfg* cfg, ptx_worker_event* info /* NULL ok */);

/* Same, from caller-provided arrays (procedural scenes, or a host that did its own parsing).
 * Models are given in the order the reference's renderer::intersect would visit them. */
typedef struct ptx_scene_desc {
	uint32_t n_models;
	const float* model_xform;    /* [n_models][12]: origin(3), basis.x(3), basis.y(3), basis.z(3) — scene::transform */
	const int32_t* model_surf;   /* [n_models][2]: first surface, surface count — scene::model::surfaces */
	uint32_t n_surfaces;
	const int32_t* surf_range;   /* [n_surfaces][4]: first vertex, vertex count, first triangle, triangle count */
	const float* vertices;       /* [.][11]: position(3) tex_coord(2) normal(3) tangent(3) — core::vertex */
	const uint32_t* triangles;   /* [.][3]: mesh-local vertex ids — core::mesh::triangles */
	const float* materials;      /* [n_surfaces][11]: albedo(3) opacity roughness metallic emissive(3) ior shadow_catcher */
	const float* camera;         /* [13]: origin(3) basis(9) vertical fov (radians) */
	const float* sun;            /* NULL, or [13]: basis(9) energy(3) angular_radius — scene::sun_light */
} ptx_scene_desc;
int ptx_scene_from_arrays(ptx_ctx* ctx, const ptx_scene_desc* desc, ptx_scene** out);
void ptx_scene_destroy(ptx_scene* scene);

/* renderer::environment (LIB/core/renderer.hpp:28: std::shared_ptr<image::texture>, sampled on a miss through
 * core::equirectangular_proj, renderer.cpp:443-449 / shading_worker.cpp:28-35) = image_texture::load(png_path, srgb).
 * The miss colour becomes texture(dir) * environment_factor. png_path == NULL removes the map. The file may be a PNG, a JPEG or a
 * Radiance .hdr (by content, as stb_image decides); an .hdr keeps its float texels (image::hdr). */
int ptx_scene_set_environment(ptx_scene* scene, const char* png_path, int srgb);

/* ---- moving a loaded scene ------------------------------------------------------------------------
 * The camera and the model transforms of a scene can be set after creation; neither call builds a KD tree (the trees are mesh-local).
 *
 * THE CAMERA. origin, basis and yfov are ptx_scene_desc::camera [13], same order and meaning; tan_half_fov = std::tan(yfov * 0.5F) as at
 * creation. PTX_ARR_CAMERA reports the new values. The call works on host-only scenes. On a scene with a context it waits for no render
 * and re-uploads nothing but the aperture table: the camera is a kernel argument of the next launch. PTX_ERR_INVALID for a NULL argument,
 * a non-finite field, yfov outside (0, pi), lens_radius < 0, lens_radius > 0 with focus_distance not > 0, blades other than 0 or 3 .. 32;
 * decided before any device work, and a refused call leaves the camera as it was. With lens_radius == 0 the other lens fields are ignored
 * and stored as 0: the scene renders every bit as a scene never given a lens.
 *
 * THE APERTURE TABLE (PTX_ARR_LENS): float[blades + 1][2], empty while lens_radius == 0. Built on the host in float64 from the stored
 * float32 fields and stored as float32: v_k = (R cos th_k, R sin th_k), th_k = blade_rotation + 2 pi k / blades, k = 0 .. blades - 1;
 * entry `blades` is a bitwise copy of entry 0.
 *
 * THE LENS: what every integrator's camera sample computes (ptx_render with both integrators, ptx_render_transparent, ptx_render_aov,
 * ptx_render_nee in both forms, both adaptive calls). IEEE binary32, each operation rounded on its own, in the order written; normalize
 * and mulmv are the device's own, as scene::camera::get_ray uses them.
 *   j = draws(pixel, sample, 0, 0, BLOCK_JITTER); j.x, j.y are the pixel jitter (the worker estimator's un-jittered sample 0 zeroes j.x,
 *   j.y only); ndc_x, ndc_y, ratio, dx, dy and dir = normalize((dx, dy, -1)) as in camera::get_ray.
 *   lens_radius == 0: o and d as camera::get_ray gives them.
 *   lens_radius > 0, n = blades, v = the aperture table:
 *     t = focus_distance / (0 - dir.z);   pf = dir * t
 *     a = j.z * (float)n;   k = min((uint32_t)a, n - 1);   u = a - (float)k;   su = sqrt(u)
 *     beta = su * (1 - j.w);   gamma = su * j.w
 *     lx = beta * v[k].x + gamma * v[k+1].x;   ly = beta * v[k].y + gamma * v[k+1].y;   lp = (lx, ly, 0)
 *     dl = normalize(pf - lp);   o = mulmv(basis, lp) + origin;   d = normalize(mulmv(basis, dl))
 *   The lens point is uniform on the polygon (E[|lp|^2] = R^2 (2 + cos(2 pi / n)) / 6), and every lens ray of one (ndc_x, ndc_y) passes
 *   through pf, the pinhole ray's point on the plane of focus. ptx_render_aov's depth is the distance from the sample's own lens point. */
typedef struct ptx_camera {
	float origin[3]; float basis[9]; float yfov;
	float lens_radius;      /* circumradius of the aperture, scene units; 0 = pinhole */
	float focus_distance;   /* distance of the plane of focus in front of the camera, along its -Z axis */
	uint32_t blades;        /* the aperture is a regular polygon of 3 .. 32 corners; 0 = 16 */
	float blade_rotation;   /* radians, angle of corner 0 from the camera's +X axis */
} ptx_camera;
int ptx_scene_set_camera(ptx_scene* scene, const ptx_camera* camera);
/* as stored: blades resolved, the lens fields 0 on a scene never given a lens */
int ptx_scene_get_camera(const ptx_scene* scene, ptx_camera* camera);

/* THE MODEL TRANSFORMS, in the layout and order of PTX_ARR_MODEL_XFORM. Afterwards the scene is indistinguishable from one created by
 * ptx_scene_from_arrays from the same arrays with these transforms: every ptx_scene_get_array, ptx_scene_get_info and every render is
 * bitwise equal. The model, ray-space and shade records are recomputed; the light list of ptx_render_nee is dropped and rebuilt at the
 * next request; on a scene with a context the records go up again into the buffers the scene owns. The environment map, the punctual
 * lights (world-space state: they do not move with models) and the camera stay as set. Works on host-only scenes. PTX_ERR_INVALID for a
 * NULL argument, n_models different from the scene's, and a non-finite value; decided before the scene is touched. */
int ptx_scene_set_model_xforms(ptx_scene* scene, const float* model_xform /* [n_models][12], host */, uint32_t n_models);

/* MOTION: a shutter over moving models and a moving camera. The scene as it stands (its current camera and current transforms) is the
 * state at u = 1; `m` gives the state at u = 0, in the shape of ptx_motion_prev on purpose: a frame loop hands the same previous-frame
 * arrays to both calls. m == NULL clears the motion.
 *
 * WHICH MODELS MOVE. A model whose 12 begin floats are bitwise equal to its current ones is static, and so is a camera whose begin origin
 * and basis are bitwise equal to the current ones (the begin camera's yfov and lens fields are ignored; the current camera's hold).
 * Nothing is ever interpolated for a static model or camera. If no model and no camera moves the motion is INACTIVE: every call runs
 * exactly as on a scene never given motion, kernels and PTX_NEE_FUSED included.
 *
 * LIFETIME. ptx_scene_set_model_xforms and ptx_scene_set_camera clear the motion, so the order within a frame is: the two setters first,
 * ptx_scene_set_motion last. The call works on host-only scenes. On a scene with a context it uploads one small table (begin and current
 * transforms, moved flags) and the ray spaces into buffers the scene owns; it drops the light list and builds no tree.
 *
 * REFUSALS, all PTX_ERR_INVALID and decided before the scene is touched (a refused call leaves the motion as it was): a NULL scene;
 * n_models different from the scene's when transforms are given; a non-finite value; a begin camera that ptx_scene_set_camera would refuse
 * on its origin, basis or yfov; a shutter value that is NaN or outside 0 <= open <= close <= 1.
 *
 * THE SPECIFICATION. IEEE binary32, each operation rounded on its own, in the order written.
 *   Time of a sample:  r = draws(pixel, sample, 0, 0, BLOCK_TIME = 0x300).x;  u = shutter_open + (shutter_close - shutter_open) * r.
 *     u is a function of (seed, pixel, sample) alone; the camera ray and every ray of the sample's path carry it: continuation,
 *     pass-through, sun, light and punctual shadow rays.
 *   State at u:  for a moving model x(u)[k] = a[k] + (b[k] - a[k]) * u for the 12 floats, a the begin and b the current value; the camera's
 *     origin and basis follow the same formula. The derived records are those of ptx_scene_set_model_xforms, operation for operation:
 *     inv_basis = inverse(basis) (mat3 inverse: cofactors times 1 / det), inv_origin = inv_basis * (-origin), nmat = the transposed
 *     inverse. One function computes them on the host and in the kernels. A static model's records are the scene's own, read without
 *     arithmetic. (x(1) is what the formula gives; it need not be b bit for bit.)
 *   Consequence, which the tests hold on to: a ray of time u sees, bit for bit, the scene set with ptx_scene_set_model_xforms(x(u)) and no
 *     motion; and with shutter_open == shutter_close == u every sample has time exactly u.
 *   A linear blend of two rotations shrinks in between and can be singular (a half-turn at u = 0.5 is). Nothing special is done: the
 *     frame is what the static scene with that matrix renders. Subdivide large rotations into several frames' keys.
 *   The light list: a surface of a moving model is not listed. An emitter on a moving model keeps emission weight 1 and receives no light
 *     samples (the rule for unlisted emitters: nothing is lost or counted twice). Clearing the motion lists it again.
 *   Ray spaces: two models share a local ray when their current inverse transforms are bitwise equal and neither moves; two moving models
 *     only when their begin and current transforms are both bitwise equal. Models that meet at u = 1 from different begin states do not.
 *
 * INSPECTION. PTX_ARR_MOTION_XFORM, PTX_ARR_MOTION_MOVED, PTX_ARR_MOTION_CAMERA (below); all three are empty when no motion is set.
 * ptx_scene_motion_state evaluates the state at u with the one function the kernels use: model_xform [n_models][12] and camera [12]
 * (origin, basis); either may be NULL; works on host-only scenes; PTX_ERR_INVALID for a NULL scene or a non-finite u.
 *
 * WHAT RUNS UNDER ACTIVE MOTION.
 *   ptx_render_nee and ptx_render_adaptive_nee run their unfused form: k_nee_generate computes u, the camera at u and the camera ray;
 *     every closest-hit and shadow batch of a round carries the times; k_nee_shade takes the hit surface's records at u. PTX_NEE_FUSED is
 *     ignored exactly as on the queue route (fused_launches == 0), not refused. Tiles, sample ranges, spp_per_pass, shards and the adaptive
 *     loop compose bit for bit as without motion. With PTX_NEE_NO_LIGHT_SAMPLES this is ptx_render's estimator under the shutter.
 *   With PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION on a scene of the fused route they run ONE launch per pass of a fused kernel that carries a
 *     time per lane (k_nee_fused_motion): a lane that starts a sample computes u, blends the camera for itself, traces every ray of the
 *     path at u and takes a moving hit surface's records at u. accum and the stats are bit for bit the unfused form's under the same
 *     motion (PTX_NEE_FUSED_MOTION below). PTX_NEE_NO_LIGHT_SAMPLES | PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION is ptx_render's estimator
 *     under a shutter in one launch per pass.
 *   ptx_render_aov: the same camera sample and time, with depth measured from the lens point of the camera at u: the guides of the
 *     blurred frame, which is what ptx_denoise needs for it.
 *   ptx_intersect_batch_motion (below ptx_intersect_batch) takes a time per ray on every route.
 *   Refused with PTX_ERR_UNSUPPORTED before any device work, the message naming ptx_render_nee: ptx_render, ptx_render_transparent,
 *     ptx_render_adaptive, ptx_render_motion, ptx_render_emission, and every call with PTX_INTEGRATOR_WORKER. The project refuses rather
 *     than render a frame with an instantaneous shutter where a blurred one was asked for. With inactive or cleared motion all of them run
 *     as before.
 *
 * OUT OF SCOPE: more than two keys and curved paths; vertex animation; motion in ptx_render's fused kernel (k_render_pass: ptx_render keeps
 * refusing; PTX_NEE_FUSED alone stays ignored under active motion and needs PTX_NEE_FUSED_MOTION beside it) and in the worker estimator; light samples towards moving emitters; ptx_render_motion and ptx_render_emission under a shutter, and with them the
 * temporal filters on blurred frames; stratified time samples; a moving sun, environment or punctual lights. */
typedef struct ptx_motion {
	const ptx_camera* begin_camera;    /* NULL: the camera does not move */
	const float* begin_model_xform;    /* NULL: no model moves; else [n_models][12], host, layout of PTX_ARR_MODEL_XFORM */
	uint32_t n_models;
	float shutter_open, shutter_close; /* 0 <= open <= close <= 1 */
} ptx_motion;
int ptx_scene_set_motion(ptx_scene* scene, const ptx_motion* m /* NULL clears */);
int ptx_scene_motion_state(const ptx_scene* scene, float u, float* model_xform /* [n_models][12] or NULL */, float* camera /* [12] or NULL */);

/* Point and spot lights (glTF KHR_lights_punctual; no counterpart in the reference, which reads only the `directional` sun). They are
 * scene state that ptx_render_nee and ptx_render_adaptive_nee sample as a third light-sampling strategy (PUNCTUAL LIGHTS below
 * ptx_render_nee's flags has the estimator); ptx_render, ptx_render_transparent, ptx_render_aov and the PTX_INTEGRATOR_WORKER estimator
 * ignore them. A light is a record of 16 floats:
 *   [0..2] position   [3] range (0 = unlimited)   [4..6] direction: the unit direction the light shines in (ignored for a point light)
 *   [7] kind: 0 point, 1 spot   [8..10] intensity rgb = colour x intensity   [11] cos_inner   [12] cos_outer   [13..15] zero
 * n = 0 (lights may be NULL) removes them. Works on host-only scenes too; the call does no device work. PTX_ERR_INVALID for a NULL scene,
 * NULL lights with n > 0, n > 65536, a non-finite field, a kind other than 0 or 1, a negative intensity component or range, a spot whose
 * direction is not within 1e-3 of unit length, and a spot with cos_inner < cos_outer; a refused call leaves the scene's lights as they were.
 *   THE CDF (PTX_ARR_PUNCTUAL_CDF), built on the host in float64 and stored as float32: the cumulative share of
 *     lum(intensity) = 0.2126 r + 0.7152 g + 0.0722 b, the last entry 1. A light of zero luminance has probability 0; if all have, the call
 *     stores no lights, exactly as n = 0. pmf_k is the difference of the STORED entries with cdf[-1] = 0: the probability the sampler realises. */
int ptx_scene_set_punctual_lights(ptx_scene* scene, const float* lights /* [n][16], host */, uint32_t n);
/* The `point` and `spot` lights of a glTF file as records for ptx_scene_set_punctual_lights. Host only, no context; only the .gltf is read.
 * One record per node of scenes[0] that references such a light, in the loader's pre-order, placed by the loader's own node transforms
 * (TRS only): position = the node's world origin, direction = the normalised world image of the local -Z axis, intensity = color (default
 * 1, 1, 1) x intensity (default 1), range default 0, cos_inner = cos(innerConeAngle) (default 0), cos_outer = cos(outerConeAngle) (default
 * pi / 4), computed in float64 and stored as float32 (a point light's are the defaults'). `directional` lights are skipped: the sun stays
 * where it is (ptx_load_opts::sun_light_index). Returns the number of records; dst == NULL only counts. Returns -(ptx_status) on a file or
 * parse error and when dst_floats < 16 x the count. ptx_scene_load_gltf does not pick the lights up: the caller reads and sets them. */
int64_t ptx_gltf_read_punctual_lights(const char* gltf_path, float* dst /* NULL = count only */, size_t dst_floats);
/* How a punctual sample picks its light (PUNCTUAL PICK below ptx_render_nee's flags has the tree, the importance and the descent):
 * PTX_PUNCTUAL_PICK_CDF, the default, from the CDF over lum(intensity), whatever the shading point; PTX_PUNCTUAL_PICK_TREE by a stochastic
 * descent of a binary tree over the lights with importance power / distance^2 seen from the shading point. Opt-in scene state: a scene on
 * which the setter was never called, or was last called with CDF, renders every bit as before. Works on host-only scenes and does no device
 * work; the tree (PTX_ARR_PUNCTUAL_TREE) is built by the call from the stored lights, rebuilt by every later ptx_scene_set_punctual_lights
 * (the mode survives a new light set and a clear) and uploaded at the first render after a change, as the records and the CDF are.
 * ptx_scene_set_model_xforms, ptx_scene_set_camera and ptx_scene_set_motion leave mode and tree alone: lights are world-space state.
 * PTX_ERR_INVALID for a NULL scene (or a NULL `pick` of the getter) and for an unknown mode; a refused call leaves the mode as it was. */
typedef enum ptx_punctual_pick { PTX_PUNCTUAL_PICK_CDF = 0, PTX_PUNCTUAL_PICK_TREE = 1 } ptx_punctual_pick;
int ptx_scene_set_punctual_pick(ptx_scene* scene, uint32_t pick);
int ptx_scene_get_punctual_pick(const ptx_scene* scene, uint32_t* pick);
/* How a light sample picks its emissive triangle (LIGHT PICK below ptx_render_nee's flags has the tree, the importance, the descent and what
 * changes in the estimator): PTX_LIGHT_PICK_CDF, the default, from the CDF over area, whatever the shading point; PTX_LIGHT_PICK_TREE by a
 * stochastic descent of a binary tree over the light list with importance power / distance^2 seen from the shading point. Opt-in scene
 * state, independent of the punctual mode: a scene on which the setter was never called, or was last called with CDF, runs the same kernels
 * and renders every bit as before. Works on host-only scenes and does no device work. The mode outlives the light list: the tree
 * (PTX_ARR_LIGHT_TREE, PTX_ARR_LIGHT_PATH) is built together with the list at the first request, dropped with it by whatever drops the list
 * (ptx_scene_set_model_xforms, ptx_scene_set_motion both ways, and a change of this mode), rebuilt with it and uploaded with it.
 * PTX_ERR_INVALID for a NULL scene (or a NULL `pick` of the getter) and for an unknown mode; a refused call leaves the mode as it was. */
typedef enum ptx_light_pick { PTX_LIGHT_PICK_CDF = 0, PTX_LIGHT_PICK_TREE = 1 } ptx_light_pick;
int ptx_scene_set_light_pick(ptx_scene* scene, uint32_t pick);
int ptx_scene_get_light_pick(const ptx_scene* scene, uint32_t* pick);

typedef struct ptx_scene_info {
	uint32_t n_models, n_surfaces, n_vertices, n_triangles;
	uint32_t n_kd_nodes;      /* flattened 8-byte nodes (branches + leaves) */
	uint32_t n_kd_refs;       /* leaf triangle references */
	uint32_t kd_max_depth;
	uint32_t has_sun;
	uint32_t geometry_bytes;  /* nodes + refs + triangle records: what the kernels stage through LDS */
	uint32_t lds_resident;    /* where the kernels read KD nodes / triangle records from: 0 = L2/HBM, 1 = all of it staged in
	                           * each CU's LDS, 2 = hybrid (the surfaces that fit in LDS, the large ones in L2/HBM) */
	uint32_t n_textures;
} ptx_scene_info;
int ptx_scene_get_info(const ptx_scene* scene, ptx_scene_info* info);

/* Host copies of the flattened arrays (tests, tooling). Returns the element count; dst may be NULL
 * to query it. Element layouts are documented in DESIGN.md §"Data layout". */
typedef enum ptx_array {
	PTX_ARR_MODEL_XFORM = 0,  /* float[n_models][12] */
	PTX_ARR_MODEL_AABB = 1,   /* float[n_models][6]  */
	PTX_ARR_MODEL_SURF = 2,   /* int32[n_models][2]  */
	PTX_ARR_SURF_RANGE = 3,   /* int32[n_surfaces][8]: v0,nv,t0,nt,kd_root,n_nodes,ref0,n_refs */
	PTX_ARR_MESH_AABB = 4,    /* float[n_surfaces][6] */
	PTX_ARR_VERTICES = 5,     /* float[n_vertices][11] */
	PTX_ARR_TRIANGLES = 6,    /* uint32[n_triangles][3] */
	PTX_ARR_MATERIALS = 7,    /* float[n_surfaces][11] */
	PTX_ARR_KD_NODES = 8,     /* uint32[n_kd_nodes][2]  (packed device nodes) */
	PTX_ARR_KD_REFS = 9,      /* uint32[n_kd_refs]      (global triangle ids) */
	PTX_ARR_CAMERA = 10,      /* float[14]: origin basis fov tan_half_fov */
	PTX_ARR_SUN = 11,         /* float[13] or empty */
	PTX_ARR_MODEL_NAMES = 12, /* char[]: '\n'-separated entity names in visit order */
	PTX_ARR_TEXTURES = 13,    /* uint32[n_textures][4]: width, height, channels | srgb << 8 | float << 16, byte offset into TEXELS (float offset into TEXELS_F32) */
	PTX_ARR_TEXELS = 14,      /* uint8[]: 8-bit texels of all textures (rows top to bottom, as decoded) */
	PTX_ARR_SURF_TEX = 15,    /* int32[n_surfaces][7]: texture id per material slot (normal, albedo, opacity, occlusion, roughness, metallic, emissive), -1 = none */
	PTX_ARR_TEXELS_F32 = 16,  /* float[]: texels of Radiance .hdr images (TEXTURES entries with bit 16 of the third word; their offset counts floats here) */
	/* the light list of ptx_render_nee (built at the first request, on host-only scenes too) */
	PTX_ARR_LIGHT_TRIS = 17,  /* uint32[n_lights][2]: surface, triangle index within the surface's mesh */
	PTX_ARR_LIGHT_CDF = 18,   /* float[n_lights]: cumulative share of the listed area, the last entry 1 */
	PTX_ARR_LIGHT_GEOM = 19,  /* float[n_lights][4]: geometric normal (world), area (world) */
	/* the LDS residency plan (read-only; what the fused kernels stage into each CU's LDS) */
	PTX_ARR_TRI_ISECT = 20,   /* uint32[n_triangles][12]: the 48-byte intersection records, one per triangle (bit patterns; word 10 = triangle id,
	                           * on an uploaded scene | hot-record slot << 24) */
	PTX_ARR_RES_NODES = 21,   /* uint32[.][2]: KD nodes of the resident surfaces; a leaf's first word indexes RES_REFS (ref-indexed surface)
	                           * or RES_TRIS (leaf-ordered surface) */
	PTX_ARR_RES_REFS = 22,    /* uint32[.]: leaf references of the ref-indexed resident surfaces, indices into RES_TRIS */
	PTX_ARR_RES_TRIS = 23,    /* uint32[.][12]: resident records: one per triangle (ref-indexed surface) or per leaf reference (leaf-ordered) */
	PTX_ARR_LDS_ROOT = 24,    /* uint32[n_surfaces]: 0xFFFFFFFF = not resident, else root index in RES_NODES | leaf-ordered << 31 */
	PTX_ARR_RES_PLAN = 25,    /* uint32[4]: bytes of the resident arrays + shade records, resident surfaces, dynamic LDS bytes of the fused
	                           * kernels (0 on a host-only scene), hot hit records */
	/* the environment map's sampling table of PTX_NEE_ENV_SAMPLES (built at the first request, on host-only scenes too; both empty when the
	 * scene has no map or the map is black; ptx_scene_set_environment drops the table) */
	PTX_ARR_ENV_ROW_CDF = 26, /* float[h]: cumulative share of the rows' mass, top row first, the last entry 1 */
	PTX_ARR_ENV_CELL_CDF = 27,/* float[h][w]: cumulative share of the boxes within their row, the last entry 1; a row of zero mass is all 0 */
	/* the punctual lights of ptx_scene_set_punctual_lights (host-only scenes too; both empty when none are set) */
	PTX_ARR_PUNCTUAL = 28,    /* float[n][16], as stored */
	PTX_ARR_PUNCTUAL_CDF = 29,/* float[n]: cumulative share of lum(intensity), the last entry 1 */
	PTX_ARR_LENS = 30,        /* float[blades + 1][2]: the aperture table of ptx_scene_set_camera; empty while lens_radius == 0 */
	PTX_ARR_LDS_SHAPE = 31,   /* uint32[n_surfaces]: the surface records' whole lds_root word: LDS_ROOT's (root in bits 28:0) | leaf-only tree << 30 |
	                           * complete tree of at most 3 branch levels << 29 (the shape bits: leaf-ordered surfaces only, none with PTX_KD_SHAPES=0) */
	PTX_ARR_SURF_AUX = 32,    /* uint32[n_surfaces][4]: the auxiliary surface records: word 0 = flags, bit 0 = the resident, leaf-ordered tree is a
	                           * chain: every branch has exactly one child, down to a leaf (none with PTX_KD_SHAPES=0); words 1-3 are padding */
	/* the motion of ptx_scene_set_motion (host-only scenes too); all three empty when no motion is set */
	PTX_ARR_MOTION_XFORM = 33, /* float[n_models][12]: the begin transforms; a static model's entry is its current transform */
	PTX_ARR_MOTION_MOVED = 34, /* uint32[n_models]: 1 = the model moves */
	PTX_ARR_MOTION_CAMERA = 35,/* float[15]: begin origin, begin basis (the current camera's when it does not move), camera-moved flag, open, close */
	/* the light tree of ptx_scene_set_punctual_pick (host-only scenes too) */
	PTX_ARR_PUNCTUAL_TREE = 36,/* uint32[n_nodes][8], bit patterns: lo.xyz, power, hi.xyz, word 7; empty in CDF mode and without lights */
	/* the light tree over the light list of ptx_scene_set_light_pick (built with the list, on host-only scenes too; both empty in CDF mode
	 * and with an empty list) */
	PTX_ARR_LIGHT_TREE = 37,   /* uint32[n_nodes][8], bit patterns: lo.xyz, power, hi.xyz, word 7 (LIGHT PICK below ptx_render_nee's flags) */
	PTX_ARR_LIGHT_PATH = 38    /* uint32[n_lights]: the path word of each listed triangle: bit i = step i of the descent to its leaf goes right */
} ptx_array;
int64_t ptx_scene_get_array(const ptx_scene* scene, ptx_array which, void* dst, size_t dst_bytes);

/* ---- tile worker --------------------------------------------------------------------------------
 * Replaces core::renderer::render() (LIB/core/renderer.hpp:36, renderer.cpp:334-428) and the worker's
 * staged pipeline (src/processors/worker/worker.hpp:27-41): renders samples [sample0, sample0+spp) of
 * the pixel rectangle [x0,x0+w) x [y0,y0+h) of a W x H image and ADDS the per-pixel radiance SUMS
 * (not means) into accum_rgba[h][w][4] (float32; alpha accumulates 1 per sample, as renderer.cpp:398).
 * The fields mirror core::renderer's public fields (renderer.hpp:21-33) with the same defaults.
 * Random numbers are a counter-based Philox4x32-10 stream keyed by (seed, pixel y*W+x, sample index,
 * depth, draw), so any tiling / sample split / GPU count gives the same per-sample radiance. */
/* Which of the reference's two estimators one sample runs.
 * PTX_INTEGRATOR_LIB:    core::renderer::trace (LIB/core/renderer.cpp:437-643) — what `path_tracer_lib` and its example
 *                        program render with; pinned against the compiled reference (oracle/_ref).
 * PTX_INTEGRATOR_WORKER: the HOST worker's stage pipeline for one worker — INTERSECT -> DIRECT_LIGHTING -> SHADING ->
 *                        ACCUMULATE (src/processors/worker/intersection_worker.cpp:10-67, shading_worker.cpp:10-201,
 *                        worker.cpp:114-149): emissive added before the opacity test, throughput clamped to [0,10],
 *                        Russian roulette once bounce < bounce_count-2, un-jittered sample 0, and a shadow catcher that
 *                        is black unless its sun sample is unoccluded. Pinned: the oracle the kernels are tested against replays
 *                        the compiled worker stages' own random streams bit for bit, and the un-jittered first sample at one
 *                        bounce is compared with compiled worker output at zero tolerance (tests/test_worker_pin.py). Not
 *                        replicated: entity visit order on exact distance ties between models, thread timing, and
 *                        bounce_count = 0 (the reference's uint8_t bounce wraps; here the render is black). */
typedef enum ptx_integrator { PTX_INTEGRATOR_LIB = 0, PTX_INTEGRATOR_WORKER = 1 } ptx_integrator;
typedef struct ptx_render_cfg {
	uint32_t W, H;          /* renderer::resolution (1920 x 1080) */
	uint32_t spp;           /* renderer::sample_count */
	uint32_t bounces;       /* renderer::bounce_count (4) */
	float env[3];           /* renderer::environment_factor (1,1,1) */
	uint32_t seed_lo, seed_hi;
	uint32_t x0, y0, w, h;  /* tile; w = h = 0 means the whole image */
	uint32_t sample0;       /* first sample index */
	uint32_t spp_per_pass;  /* 0 = library default; samples of every pixel traced per kernel launch */
	uint32_t integrator;    /* ptx_integrator */
	/* Interleaved tile sharding (one frame split over several GPUs / workers): when shard_count > 1, only
	 * the pixels of the rectangle that lie in image tiles t with t % shard_count == shard_index are rendered, where t is the
	 * row-major index of the shard_tile x shard_tile tile of the FULL W x H image that holds the pixel (shard_tile 0 = 64).
	 * accum keeps the [h][w] layout of the rectangle; pixels of other shards are left untouched, so the sum of all shards'
	 * buffers (x + 0 = x) is bitwise the unsharded frame. shard_count 0 or 1 = no sharding. */
	uint32_t shard_index, shard_count, shard_tile;
} ptx_render_cfg;
typedef struct ptx_render_stats {
	uint64_t rays;          /* closest-hit + shadow queries = renderer::intersect calls (renderer.cpp:441,509) */
	uint64_t samples;       /* camera paths = trace() root calls */
	uint64_t passes;        /* kernel launches of the integrator */
	double kernel_ms;       /* HIP-event time of the integrator kernels on the context stream */
} ptx_render_stats;
/* accum_rgba: device or host pointer. stats may be NULL (no device->host sync is then forced). */
int ptx_render(ptx_scene* scene, const ptx_render_cfg* cfg, float* accum_rgba, ptx_render_stats* stats);

/* core::renderer::render() with transparent_background = true (renderer.cpp:340-399, :444), PTX_INTEGRATOR_LIB only.
 * A sample's alpha is 0 when trace()'s top-level return is a miss — the camera ray missed, or the ray continued behind an opacity /
 * lit shadow-catcher pass-through did (renderer.cpp:471, 518) — and 1 for every other ending. The reference then blends the samples
 * of a pixel IN SAMPLE ORDER on the state {color, alpha, claimed} (renderer.cpp:374-399): the first opaque sample s claims the pixel
 * (color = sample, alpha = 1 / (s + 1) in INTEGER arithmetic: 1 for s = 0, else 0 — kept as the reference has it); a transparent
 * sample changes only the alpha of a claimed pixel and nothing of an unclaimed one; an opaque sample on a claimed pixel takes the
 * running mean of colour and alpha. pixel_rgba[h][w][4] (float32) holds that running color / alpha — MEANS, not sums — and
 * claimed[h][w] (one byte per pixel, 0 / 1) the flag; both device or both host. The call advances them through samples
 * [sample0, sample0 + spp) of the rectangle. A frame starts from zeroed buffers at sample0 = 0.
 * The blend is a recurrence, not a sum. What composes: calls of ASCENDING, adjacent sample ranges on the same buffers (bitwise the
 * frame of one call, for any spp_per_pass); tile rectangles; shard_* as in ptx_render — other shards' pixels stay as they were, so
 * the sum of the shards' zero-initialised buffers is bitwise the unsharded frame. What does NOT: sample ranges of one frame rendered
 * into independent buffers cannot be merged afterwards — split a frame over GPUs by tiles or shards in this mode.
 * Image write: ptx_tonemap_encode(ctx, pixel_rgba, W, H, 1, rgba8) is the reference's write loop for these means (x / 1.0f is exact;
 * alpha is quantised without sRGB, image.cpp:143-154).
 * PTX_ERR_UNSUPPORTED for PTX_INTEGRATOR_WORKER (the worker's alpha is that of the path's last vertex, shading_worker.cpp:36,43, and it
 * jitters sample 0 in this mode, worker.cpp:125: nothing pins it); PTX_ERR_NO_DEVICE for a host-only scene; PTX_ERR_INVALID for NULL
 * buffers — all decided before any device work. */
int ptx_render_transparent(ptx_scene* scene, const ptx_render_cfg* cfg, float* pixel_rgba, uint8_t* claimed, ptx_render_stats* stats);

/* First-hit guide buffers for a denoiser (no counterpart in the reference, which writes the beauty frame only): per camera sample, the albedo,
 * world shading normal and depth of the first surface the sample ends on, and whether it ends on one (coverage). The camera samples are
 * exactly those of ptx_render: the same cfg fields (W, H, x0, y0, w, h, sample0, spp, seed_*, spp_per_pass, shard_*) and the same Philox
 * keys, so sample s of pixel p here is the camera ray of sample s of pixel p in the beauty frame (renderer.cpp:359-370). `bounces` and
 * `env` are ignored.
 * One sample: the camera ray goes through renderer::intersect (renderer.cpp:441). On a hit the material is evaluated (renderer.cpp:458-463)
 * and the opacity rule of renderer.cpp:466-472 applied as the integrator applies it — !is_approx(opacity, 1) && draw > opacity, with the
 * integrator's own draw for that vertex (depth 0, the sample's pass count) — and a sample that passes through continues from
 * position + dir * epsilon with the re-normalised direction; after 4096 pass-throughs it ends as a miss, as in ptx_render. The first
 * vertex that does not pass through is the sample's surface: albedo = material::get_albedo, normal = intersect_result::get_normal()
 * (renderer.cpp:430-435, what ptx_hits.nx/ny/nz report), depth = length(position - origin of the camera ray). A back-facing hit
 * (renderer.cpp:478) is recorded like any other. A shadow catcher is an ordinary surface here: whether it passes a sample through depends
 * on its sun sample (renderer.cpp:513-519), which stays with the beauty path. A miss adds nothing to either buffer.
 * Both buffers are SUMS over the samples, ADDED to what the caller passes in; a pixel's samples are added in sample order. So calls of
 * ASCENDING, adjacent sample ranges on the same buffers are bitwise one call (for any spp_per_pass); tile rectangles and shard_* compose as
 * in ptx_render (other shards' pixels are untouched: the sum of zero-initialised shard buffers is bitwise the unsharded one), and
 * ptx_reduce_framebuffer applies as it is. Sample ranges rendered into separate buffers agree up to float summation order only.
 * Either pointer may be NULL (that buffer is not produced), not both; two buffers are both device or both host memory.
 * stats (may be NULL): rays = intersect queries, continuation rays included; samples; passes; kernel_ms = HIP-event time of the passes.
 * PTX_ERR_INVALID for a NULL scene, cfg or out or two NULL buffers; PTX_ERR_UNSUPPORTED for PTX_INTEGRATOR_WORKER (its opacity handling,
 * shading_worker.cpp:54-63, and un-jittered sample 0, worker.cpp:125-126, are not pinned); PTX_ERR_NO_DEVICE for a host-only scene —
 * all decided before any device work. */
typedef struct ptx_aov_buffers {
	float* albedo_cov;    /* [h][w][4]: sum of albedo rgb over the samples that end on a surface; w = how many did (coverage count) */
	float* normal_depth;  /* [h][w][4]: sum of the world shading normal xyz; w = sum of length(hit position - camera ray origin) */
} ptx_aov_buffers;
int ptx_render_aov(ptx_scene* scene, const ptx_render_cfg* cfg, const ptx_aov_buffers* out, ptx_render_stats* stats);

/* Per-sample screen-space motion for temporal reprojection (ptx_denoise_temporal; no counterpart in the reference): where on the PREVIOUS
 * frame's screen the surface point of each camera sample was, given the previous camera and the previous model transforms. The scene is the
 * current frame's (ptx_scene_set_camera, ptx_scene_set_model_xforms); `prev` is what the caller set one frame earlier.
 * The camera samples, the walk through opacity pass-throughs (pass + 1, the 4096 bound) and the rule "the first vertex that does not pass
 * through is the sample's surface" are ptx_render_aov's, word for word: the same cfg fields, the same Philox keys, the same intersect route.
 * Per sample that ends on a surface, triangle (A, B, C) of model m, barycentrics b1, b2 (IEEE binary32, each operation rounded on its
 * own, in the order written; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; M * v = per row (m.x*v.x + m.y*v.y) + m.z*v.z):
 *   lp = A*b0 + B*b1 + C*b2 with b0 = 1 - b1 - b2 (local corners), pos = basis_m * lp + origin_m: the position ptx_hits reports.
 *   pos_prev = pos — no arithmetic — if prev or prev->model_xform is NULL or model m's 12 previous floats are bitwise equal to its current
 *   ones; else pos_prev = prev_basis_m * lp + prev_origin_m.
 *   project(cam, p): q = p - cam.origin; c = (dot(basis.x, q), dot(basis.y, q), dot(basis.z, q)) with basis.x/y/z the basis' columns;
 *     defined iff c.z < 0; iz = 0 - c.z; ndc_x = ((c.x / iz) / ratio) / tan_half_fov; ndc_y = (c.y / iz) / tan_half_fov;
 *     fx = ((ndc_x + 1) * 0.5f) * float(W); fy = ((1 - ndc_y) * 0.5f) * float(H); ratio = float(W) / float(H);
 *     tan_half_fov = std::tan(yfov * 0.5f) on the host, as at creation.
 *     This is the inverse of the camera's ray (scene::camera::get_ray) for a basis that is a rotation times a uniform scale: the camera
 *     sample through pixel position (fx, fy) sees p. Other bases are out of scope. A lens is ignored on both cameras: both projections go
 *     through the camera's centre.
 *   record = (fx_prev - fx_cur, fy_prev - fy_cur, length(pos_prev - prev_cam.origin), 1) with (fx_cur, fy_cur) = project(current camera,
 *   pos) and (fx_prev, fy_prev) = project(previous camera, pos_prev). A sample contributes nothing if either projection is undefined, or
 *   if it ends on a miss.
 * The buffer holds SUMS, ADDED to what the caller passes in; a pixel's samples are added in sample order, so tiles, ascending adjacent
 * sample ranges, spp_per_pass and shard_* compose exactly as in ptx_render_aov. .w counts the contributing samples: it equals
 * albedo_cov.w wherever every surface sample lies in front of both cameras.
 * Consequence: when nothing moved (prev NULL, or equal to the current state), .xy is exactly 0 in every pixel — identical operations on
 * identical inputs.
 * A call in which some model moved uploads the previous transforms and synchronises the context's stream once before its passes, device
 * buffers and a NULL stats included; a call in which none did synchronises as ptx_render_aov does.
 * stats as in ptx_render_aov. Refusals, all decided before any device work: everything ptx_render_aov refuses (PTX_ERR_UNSUPPORTED for
 * PTX_INTEGRATOR_WORKER, PTX_ERR_NO_DEVICE for a host-only scene, ...); PTX_ERR_INVALID for a NULL motion, for n_models different from the
 * scene's when model_xform is given, for a transform value that is not finite, and for a previous camera that ptx_scene_set_camera would
 * refuse (its lens fields are ignored). */
typedef struct ptx_motion_prev {
	const ptx_camera* camera;   /* NULL: the camera did not move (the scene's current camera is used) */
	const float* model_xform;   /* NULL: no model moved; else [n_models][12], host, layout of PTX_ARR_MODEL_XFORM */
	uint32_t n_models;
} ptx_motion_prev;
int ptx_render_motion(ptx_scene* scene, const ptx_render_cfg* cfg, const ptx_motion_prev* prev /* NULL = nothing moved */,
                      float* motion /* [h][w][4], device or host */, ptx_render_stats* stats /* NULL ok */);

/* First-hit emission (ptx_emission_split / ptx_emission_merge below; no counterpart in the reference): what every camera sample's surface
 * emits towards the camera, which is what every estimator here adds at a path's first vertex.
 * The camera samples, the walk through opacity pass-throughs (pass + 1, the 4096 bound), the rule "the first vertex that does not pass
 * through is the sample's surface" and the intersect route are ptx_render_aov's, word for word: the same cfg fields, the same Philox keys.
 * A sample that ends on a surface forms normal = the shading normal ptx_render_aov records and outcoming = -d, with d the direction of the
 * ray that found the surface (the camera ray's, or the normalised direction behind a pass-through). If
 * dot(normal, outcoming) = (n.x*o.x + n.y*o.y) + n.z*o.z > 0 the sample records (emissive10.r, emissive10.g, emissive10.b, 1), with emissive10
 * = material::get_emissive(uv) * 10 as ptx_material_eval_batch reports it (floats 9 .. 11). A back-facing surface records nothing (the
 * integrator's path ends there before its emission term, renderer.cpp:478); a miss records nothing. A shadow catcher is an ordinary surface
 * here, as in ptx_render_aov: whether ptx_render passes it through depends on its sun sample, so an emissive catcher only leaves a residual
 * for the filter.
 * The buffer holds SUMS, ADDED to what the caller passes in; a pixel's samples are added in sample order, so tiles, ascending adjacent
 * sample ranges, spp_per_pass, shard_* and host or device buffers compose exactly as in ptx_render_aov. .w counts the recording samples:
 * .w <= albedo_cov.w, with equality where no sample's surface is back-facing.
 * Consequence: on a scene without a sun (ptx_scene_info.has_sun == 0), emission.rgb is bit for bit accum.rgb of ptx_render with the same
 * cfg, bounces = 1, env = (0, 0, 0) and PTX_INTEGRATOR_LIB: at depth 0 the throughput is 1, and 1 * x and 0 + x are exact; a miss adds +0
 * there and nothing here; both add in sample order. (ptx_render_nee weights emission only at depth != 0: its first vertex adds the same.)
 * cfg->bounces and cfg->env are ignored. stats and refusals as in ptx_render_aov, all decided before any device work: PTX_ERR_UNSUPPORTED
 * for PTX_INTEGRATOR_WORKER, PTX_ERR_NO_DEVICE for a host-only scene, PTX_ERR_INVALID for a NULL scene, cfg or buffer and for whatever
 * ptx_render refuses in cfg. */
int ptx_render_emission(ptx_scene* scene, const ptx_render_cfg* cfg, float* emission /* [h][w][4], device or host */,
                        ptx_render_stats* stats /* NULL ok */);

/* Variance-guided edge-avoiding a-trous filter on the guide buffers (no counterpart in the reference, which has no denoiser): turns a noisy
 * low-spp frame into a usable one. It takes its noise estimate from two half-frames, which ptx_render gives for free — sample ranges compose.
 *   accum_a, accum_b [H][W][4]: ptx_render radiance SUMS of two disjoint sample ranges of the same frame (e.g. [0, n/2) and [n/2, n)), of
 *                               spp_a and spp_b samples;
 *   guides:                     the ptx_render_aov SUMS over all spp_a + spp_b samples; both buffers are required;
 *   out_rgba [H][W][4]:         receives MEANS (ptx_tonemap_encode(..., spp = 1, ...) writes them unchanged); may be accum_a or accum_b itself.
 * The five buffers are all device or all host memory; the filter works on whole W x H buffers, not on tiles. Multi-GPU: reduce the buffers
 * first (ptx_reduce_framebuffer applies as it is), then filter on the root.
 * The filter, which is its own specification (IEEE binary32, every operation rounded on its own in the parenthesisation written here;
 * max(a, b) returns the other operand when one is NaN):
 *   bw(x) = t * t, t = max(0, 1 - x);  lum(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b;  n = float(spp_a + spp_b), na, nb likewise.
 *   1. per pixel: cov = albedo_cov.w; alb_c = max((albedo_cov.c + (n - cov)) / n, 0.001f) (missed samples count as albedo 1);
 *      col_c = ((a.c + b.c) / n) / alb_c; ma_c = (a.c / na) / alb_c, mb_c likewise; d = (lum(ma) - lum(mb)) * 0.5f; v0 = d * d;
 *      alpha = (a.w + b.w) / n; nrm = normal_depth.xyz / cov and z = normal_depth.w / cov when cov > 0, else all 0.
 *   2. geometric weight of tap q seen from p: geo = bw(xn) * bw(xz); dn = nrm_p - nrm_q; xn = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) /
 *      (sigma_n*sigma_n); zm = max(z_p, z_q); rel = zm > 0 ? (z_p - z_q) / zm : 0; xz = (rel*rel) / (sigma_z*sigma_z). A missed pixel and
 *      a surface pixel never mix; two missed pixels mix freely.
 *   3. variance prefilter, 3 x 3, taps in row-major order (dy outer), taps outside the image skipped: g = 1 for the centre, geo otherwise;
 *      s0 += g; s1 += g * v0_q; var = s1 / s0.
 *   4. iteration i = 0 .. iterations-1, step = 2^i: the 25 taps q = p + step * (dx, dy), dy outer and dx inner from -2 to 2, taps outside
 *      the image skipped; k = {3/8, 1/4, 1/16}; h = k[|dx|] * k[|dy|]; L = lum(col); den = ((sigma_l*sigma_l) * var_p) + 1e-8f; the centre
 *      tap has w = h, any other dl = L_p - L_q and w = (h * geo) * bw((dl*dl) / den); a tap with !(w > 0) is skipped (NaN weights too: a
 *      non-finite pixel stays itself and contaminates no neighbour); acc.c += w * col_q.c; ws += w; av += (w*w) * var_q; after the taps
 *      col = acc / ws and var = av / (ws*ws).
 *   5. out.c = col.c * alb_c; out.w = alpha.
 * What to expect: the filter helps a great deal where there is noise (Cornell at 16 spp: about 4x lower mean squared error), does no harm
 * on a sun-lit open scene, and costs some texture detail on a nearly noise-free textured frame (DESIGN.md has the table).
 * PTX_ERR_INVALID — each decided before any device work — for a NULL ctx, cfg, buffer or guide pointer; W or H of 0 or above 16384; spp_a
 * or spp_b of 0; iterations above 8; a sigma that is negative or NaN; pointers of mixed kinds. */
typedef struct ptx_denoise_cfg {
	uint32_t W, H;             /* buffer size */
	uint32_t spp_a, spp_b;     /* samples summed in accum_a / accum_b; the guides hold spp_a + spp_b samples */
	uint32_t iterations;       /* 0 = 5; at most 8 (step 1, 2, 4 ... 128) */
	float sigma_l, sigma_n, sigma_z;   /* 0 = default 4, 0.5, 0.1 */
} ptx_denoise_cfg;
typedef struct ptx_denoise_stats {
	double kernel_ms;          /* HIP-event time of the filter's kernels on the context stream */
	uint32_t iterations;       /* iterations run */
	uint64_t workspace_bytes;  /* device memory the call used on the context (state buffers, and the staging of host buffers) */
} ptx_denoise_stats;
int ptx_denoise(ptx_ctx* ctx, const ptx_denoise_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, float* out_rgba,
                ptx_denoise_stats* stats /* NULL ok */);
/* ptx_denoise for half-buffers whose .w is the PER-PIXEL sample count: what ptx_render_adaptive and ptx_render_adaptive_nee leave (and what
 * ptx_render leaves too: a frame of uniform counts spp_a, spp_b with guide_spp = spp_a + spp_b is filtered bit for bit as ptx_denoise filters it).
 *   accum_a, accum_b [H][W][4]: the two halves' radiance SUMS, .w = the samples summed in that pixel;
 *   guides:                     the ptx_render_aov SUMS over guide_spp samples of EVERY pixel. For an adaptive frame render them over
 *                               [sample0, sample0 + min_spp): every pixel's samples are a prefix at least that long, so the guide samples are
 *                               camera samples of the beauty frame;
 *   out_rgba, buffer kinds, iterations, sigmas, stats: as in ptx_denoise.
 * Only step 1 of the filter's specification changes (same rounding rules); per pixel:
 *   1. na = a.w, nb = b.w, n = na + nb, ng = float(guide_spp); cov = albedo_cov.w; alb_c = max((albedo_cov.c + (ng - cov)) / ng, 0.001f);
 *      col_c = ((a.c + b.c) / n) / alb_c; ma_c = (a.c / na) / alb_c, mb_c likewise; d = (lum(ma) - lum(mb)) * 0.5f; v0 = d * d;
 *      alpha = (a.w + b.w) / n; nrm and z as in ptx_denoise.
 * Steps 2 to 5, their kernels and the workspace are ptx_denoise's. Zero counts (no adaptive frame has them: every half of a round holds a
 * sample): a pixel with n = 0 is non-finite and is treated as the filter treats every non-finite pixel — it stays itself and contaminates no
 * neighbour. A pixel with ONE empty half has a finite colour and a NaN noise estimate: the output stays finite; the pixel is never
 * filtered, and the pixels that take it as a tap inherit the NaN variance and are not filtered further.
 * PTX_ERR_INVALID, each decided before any device work, for what ptx_denoise refuses, with guide_spp == 0 in place of its spp_a / spp_b rule. */
typedef struct ptx_denoise_counts_cfg {
	uint32_t W, H;             /* buffer size */
	uint32_t guide_spp;        /* samples of every pixel summed in the guides */
	uint32_t iterations;       /* 0 = 5; at most 8 */
	float sigma_l, sigma_n, sigma_z;   /* 0 = default 4, 0.5, 0.1 */
} ptx_denoise_counts_cfg;
int ptx_denoise_counts(ptx_ctx* ctx, const ptx_denoise_counts_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides,
                       float* out_rgba, ptx_denoise_stats* stats /* NULL ok */);

/* ptx_denoise with a memory: the temporal half of SVGF in front of the filter. Last frame's integrated colour and luminance moments are
 * reprojected through per-pixel motion, rejected where the geometry disagrees, and blended with the current frame; the filter then runs on
 * the blend, with a variance taken from the integrated moments once a pixel's history is long enough. The frames of an animation stop
 * boiling, and the samples earlier frames paid for are kept.
 *   accum_a, accum_b, guides:  the current frame's two half-frame sums and its guide sums, as for ptx_denoise;
 *   motion [H][W][4]:          per pixel, SUMS over the frame's samples of (previous minus current screen position in pixels, x and y;
 *                              the surface point's distance from the previous camera; 1): the mean motion is .xy / .w, the depth the
 *                              history is expected to hold is .z / .w. A pixel with .w not > 0 has no history;
 *   prev:                      last frame's `next`, NULL for the first frame;
 *   next:                      receives this frame's history. It must not share a buffer with prev: neighbouring pixels of prev are read;
 *   out_rgba [H][W][4]:        receives MEANS, as ptx_denoise's; NULL = advance the history only (the filter is not run).
 * All buffers are device memory or all are host memory. The history holds the accumulated UNFILTERED demodulated colour: the filter's
 * output never feeds back, so its blur does not compound over the frames.
 * Only step 1 of the filter's specification changes (same rounding rules: IEEE binary32, each operation rounded on its own, in the order
 * written; max(a, b) and min(a, b) return the other operand when one is NaN). Per pixel p = (x, y):
 *   1. alb, col, v0, alpha, nrm, z: exactly step 1 of ptx_denoise. L = lum(col).
 *   2. Reprojection. No history if prev == NULL or !(motion.w > 0). Else mvx = motion.x / motion.w, mvy = motion.y / motion.w,
 *      zexp = motion.z / motion.w; gx = ((float(x) + 0.5f) + mvx) - 0.5f, gy likewise; no history unless |gx| < 32768 and |gy| < 32768
 *      (NaN fails). ix = floor(gx), wx = gx - ix; iy, wy likewise. The four taps q = (ix + dx, iy + dy), dy outer and dx inner from 0 to 1,
 *      bq = (dx ? wx : 1 - wx) * (dy ? wy : 1 - wy). A tap is taken iff it lies inside the image, bq > 0, N_q > 0 (prev.color.w),
 *      z_q > 0 (prev.geometry.w), |zexp - z_q| <= tau_z * max(zexp, z_q), and ((nrm.x*nq.x + nrm.y*nq.y) + nrm.z*nq.z) >= tau_n. A taken
 *      tap adds sw += bq and acc += bq * h_q for each of colour r, g, b, N, mu1, mu2; a tap not taken adds nothing. sw > 0: h = acc / sw,
 *      else no history. (A pixel without a surface sample has nrm = 0 and takes no tap.)
 *   3. Blend. No history: col' = col, mu1' = L, mu2' = L * L, N' = 1 (assignments). With history: N' = min(h.N + 1, float(max_history)),
 *      a = 1 / N', col' = h.col + (col - h.col) * a, mu1' = h.mu1 + (L - h.mu1) * a, mu2' = h.mu2 + (L*L - h.mu2) * a. If
 *      ((col'.r + col'.g) + col'.b) + (mu1' + mu2') is not finite the pixel starts over as one without history: no recurrence keeps a NaN.
 *   4. vf = N' < 4 ? v0 : max(0, mu2' - mu1' * mu1'); var = vf * (1 / N') — exactly v0 at N' = 1.
 *   5. next.color = (col', N'), next.moments = (mu1', mu2'), next.geometry = (nrm, z); the filter's state is (col', var), its guide
 *      (nrm, z), its re-modulation record (alb, alpha).
 * Steps 2 to 5 of the filter, their kernels and both a-trous forms are ptx_denoise's.
 * Consequences: with prev == NULL the output is bit for bit ptx_denoise's. With zero motion and a history equal to the frame (N = 1),
 * col' is bitwise col and N' = 2: one tap has weight exactly 1, the three taps of weight 0 are skipped, and col + (col - col) * a = col.
 * stats (may be NULL; NULL forces no synchronisation on device buffers): filter = ptx_denoise's stats of steps 2 to 5; accumulate_ms =
 * HIP-event time of the accumulation kernel; reprojected + reset = W * H.
 * PTX_ERR_INVALID — each decided before any device work — for what ptx_denoise refuses (out_rgba may be NULL here); a NULL motion or next
 * or member of next; a NULL member of a non-NULL prev; next sharing a buffer with prev; max_history above 1024; a tau that is negative
 * or NaN; pointers of mixed kinds. Out of scope: motion blur. Per-pixel sample counts, a wider search when all four taps fail and a
 * normal test on unit normals: ptx_denoise_temporal_counts below. */
typedef struct ptx_temporal_history {
	float* color;      /* [H][W][4]: integrated DEMODULATED colour rgb, w = history length N (float) */
	float* moments;    /* [H][W][2]: integrated first and second moment of lum(col) */
	float* geometry;   /* [H][W][4]: the frame's mean normal xyz and mean depth z, 0 for a pixel without a surface sample */
} ptx_temporal_history;
typedef struct ptx_temporal_cfg {
	uint32_t W, H, spp_a, spp_b, iterations;   /* as in ptx_denoise_cfg */
	float sigma_l, sigma_n, sigma_z;           /* as in ptx_denoise_cfg */
	uint32_t max_history;                      /* 0 = 32; at most 1024 */
	float tau_z, tau_n;                        /* 0 = 0.1, 0.9 */
} ptx_temporal_cfg;
typedef struct ptx_temporal_stats {
	ptx_denoise_stats filter;
	double accumulate_ms;
	uint64_t reprojected, reset;   /* pixels that took history / that started over */
} ptx_temporal_stats;
int ptx_denoise_temporal(ptx_ctx* ctx, const ptx_temporal_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides,
                         const float* motion, const ptx_temporal_history* prev /* NULL = first frame */, const ptx_temporal_history* next,
                         float* out_rgba /* NULL = advance the history only */, ptx_temporal_stats* stats /* NULL ok */);
/* ptx_denoise_temporal for ADAPTIVE frames: half-buffers whose .w is the per-pixel sample count (ptx_render_adaptive,
 * ptx_render_adaptive_nee), and a history whose length is counted in SAMPLES, so that a frame, or a pixel of it, weighs what it holds.
 *   accum_a, accum_b:  as for ptx_denoise_counts: the two halves' radiance SUMS, .w = the samples summed in that pixel;
 *   guides, motion:    the ptx_render_aov and ptx_render_motion SUMS over [sample0, sample0 + guide_spp) of EVERY pixel (for an adaptive
 *                      frame: over its min_spp samples), as for ptx_denoise_counts;
 *   prev, next:        as for ptx_denoise_temporal, but history.color.w counts samples. A history of ptx_denoise_temporal is not one of
 *                      this call's, nor the other way round;
 *   buffers, kinds of memory, prev == NULL, out_rgba == NULL, stats, synchronisation, the workspace and the counters: ptx_denoise_temporal's.
 * The specification is ptx_denoise_temporal's (same rounding rules) with these replacements. Per pixel p = (x, y):
 *   1. Step 1 of ptx_denoise_counts: na = a.w, nb = b.w, n = na + nb, ng = float(guide_spp); alb, col, v0, alpha, nrm, z follow from
 *      those as there. L = lum(col).
 *   2. The four bilinear taps, unchanged, and the two flags.
 *      PTX_TEMPORAL_UNIT_NORMALS: the normal test of every tap is ((u_p.x*u_q.x + u_p.y*u_q.y) + u_p.z*u_q.z) >= tau_n with
 *      u = v.xyz / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z) (three divisions by the exact square root) of nrm_p and of the tap's stored normal.
 *      A zero normal gives NaN and fails. The stored geometry and the filter's guide stay the unnormalised means. (A normal-mapped or
 *      curved pixel's mean normal is shorter than 1; against tau_n = 0.9 it cannot even match itself without this flag.)
 *      PTX_TEMPORAL_SEARCH_3X3: if the motion was usable (motion.w > 0, |gx| < 32768 and |gy| < 32768) and sw is still 0 after the
 *      four taps: rx = (int)floor(gx + 0.5f), ry likewise; the nine taps q = (rx + dx, ry + dy), dy outer and dx inner from -1 to 1. A tap
 *      is taken iff it lies inside the image, N_q > 0, z_q > 0 and it passes the same depth and normal tests. A taken tap adds sw += 1
 *      and acc += h_q (no multiplication). Then h = acc / sw if sw > 0, else no history.
 *   3. Blend. No history: col' = col, mu1' = L, mu2' = L * L, N' = n. With history: N' = min(h.N + n, max(float(max_history), n)),
 *      a = n / N', col' = h.col + (col - h.col) * a, mu1' and mu2' likewise. A blend that is not finite starts over, as before.
 *   4. vf = N' < 4 * n ? v0 : max(0, mu2' - mu1' * mu1'); var = vf * (n / N').
 *   5. As before, with next.color.w = N'.
 * Consequences. (a) With flags == 0, uniform counts spp_a, spp_b whose sum n is a power of two, guide_spp = n and max_history = n * M,
 * out_rgba, next.color.rgb, next.moments and next.geometry are bit for bit those of ptx_denoise_temporal with max_history = M, frame
 * after frame, and next.color.w is n times its value: a scaling by a power of two commutes with every rounding, and n / (n x) and 1 / x
 * round the same real number. (b) With prev == NULL the output is bit for bit ptx_denoise_counts'. (c) At zero motion over the same
 * guides the history's colour is the pooled mean of all frames' samples, up to rounding: each frame enters with weight n / N'. (d) A
 * pixel with n == 0 is non-finite, starts over every frame and is never taken as a tap (N_q > 0 fails); no adaptive frame has one.
 * max_history below n gives N' = n and a = 1: the frame replaces the history.
 * PTX_ERR_INVALID — each decided before any device work, in ptx_denoise_temporal's order — for what ptx_denoise_temporal refuses, with
 * guide_spp == 0 in place of its spp_a / spp_b rule; max_history above 1048576; a bit of flags other than the two below.
 * Out of scope: carrying history through pixels given no samples, seeding the adaptive loop from the history, transparent blends,
 * several GPUs (reduce first, as for every filter here). */
#define PTX_TEMPORAL_SEARCH_3X3   1u   /* a pixel whose four taps all fail searches the 3 x 3 texels around the rounded previous position */
#define PTX_TEMPORAL_UNIT_NORMALS 2u   /* the normal test compares directions: both mean normals are normalised first */
typedef struct ptx_temporal_counts_cfg {
	uint32_t W, H;
	uint32_t guide_spp;            /* samples of EVERY pixel summed in the guides and in motion */
	uint32_t iterations;           /* as ptx_denoise_cfg */
	float sigma_l, sigma_n, sigma_z;
	uint32_t max_history;          /* in SAMPLES; 0 = min(32 * guide_spp, 1048576); at most 1048576 */
	float tau_z, tau_n;            /* 0 = 0.1, 0.9 */
	uint32_t flags;                /* PTX_TEMPORAL_* */
} ptx_temporal_counts_cfg;
int ptx_denoise_temporal_counts(ptx_ctx* ctx, const ptx_temporal_counts_cfg* cfg, const float* accum_a, const float* accum_b,
                                const ptx_aov_buffers* guides, const float* motion, const ptx_temporal_history* prev /* NULL = first frame */,
                                const ptx_temporal_history* next, float* out_rgba /* NULL = advance the history only */,
                                ptx_temporal_stats* stats /* NULL ok */);

/* Keeping first-hit emission out of the four filter calls above. They work on radiance / albedo; on an emissive texel the radiance is not
 * proportional to the albedo texture, so the a-trous taps and the history taps would mix quotients that mean nothing once re-modulated with
 * another pixel's albedo. col = (col - e) + e is exact for any estimate e, so the emission is taken out of the half-buffers before a filter
 * call and added, unfiltered, to its output.
 *   emission [n_pixels][4]: the ptx_render_emission SUMS over guide_spp samples of EVERY pixel: all samples of a uniform frame, the min_spp
 *   prefix of an adaptive one (as the guides of ptx_denoise_counts).
 *   accum_a, accum_b [n_pixels][4]: radiance SUMS whose .w is the per-pixel sample count, as ptx_render and the adaptive calls leave them.
 *   out_rgba [n_pixels][4]: the MEANS a filter call wrote.
 * Per pixel, per channel c of r, g, b (IEEE binary32, each operation rounded on its own, in the order written, no contraction):
 *   ng = float(guide_spp);  e.c = emission.c / ng
 *   split:  if (e.c > 0) { a.c = a.c - (a.w * e.c);  b.c = b.c - (b.w * e.c); }      (b only when accum_b is given)
 *   merge:  if (e.c > 0)   out.c = out.c + e.c
 * .w of every buffer is untouched. A channel whose e.c is not > 0 (zero, negative or NaN) is left without arithmetic. Both calls work in
 * place. All pointers are device memory or all are host memory; host buffers are staged as ptx_accum_mean stages its own.
 * The pipeline: render the halves; render the guides, the emission buffer and, for the temporal calls, the motion buffer;
 * ptx_emission_split on the halves; any ONE of ptx_denoise, ptx_denoise_counts, ptx_denoise_temporal, ptx_denoise_temporal_counts,
 * unchanged: every text of theirs now reads "colour" as "colour minus e" (a negative residual is legal input: they are specified on
 * arbitrary floats); ptx_emission_merge on the filter's out_rgba. A temporal history then holds the residual: it is NOT interchangeable
 * with a history built without the split, and a sequence splits either every frame or none.
 * Consequences:
 *   (a) With an emission buffer whose rgb is all zero neither call changes a bit of any buffer, signed zeros and NaNs included.
 *   (b) On a frame with a.c = a.w * e.c + d.c and b.c = b.w * e.c - d.c, all factors dyadic so that every product and difference is
 *       exact, split, any filter call and merge return e bit for bit on every pixel where e.c > 0, whatever d, the iterations and the
 *       sigmas: the residual's sum is +0, a filter of zeros is zero, and 0 + e = e.
 * Refusals, all PTX_ERR_INVALID and all decided before any device work, the context looked at last: a NULL emission, accum_a or out_rgba;
 * guide_spp == 0; n_pixels of 0 or above 2^31 - 1; emission equal to one of the other pointers, or accum_a == accum_b; a NULL ctx; pointers of
 * mixed kinds. */
int ptx_emission_split(ptx_ctx* ctx, const float* emission, uint32_t guide_spp, size_t n_pixels, float* accum_a, float* accum_b /* NULL ok */);
int ptx_emission_merge(ptx_ctx* ctx, const float* emission, uint32_t guide_spp, size_t n_pixels, float* out_rgba);

/* Noise-driven per-pixel sample counts (no counterpart in the reference, which gives every pixel sample_count samples): a frame is rendered in
 * rounds, and a pixel whose two half-frames already agree, with all its neighbours, gets no further samples. On open, sun-lit scenes most
 * pixels stop at the first round; on a scene whose pixels are all about equally noisy (the Cornell box under this estimator, which has no
 * next-event estimation towards its area light: ptx_render_adaptive_nee below runs the same loop with it) nothing is gained over a uniform
 * frame of the same mean count (DESIGN.md has the tables).
 * There are two half-buffers, A and B: accum_a, accum_b [h][w][4] float32 radiance SUMS of the rectangle, in ptx_render's accum format (w counts
 * the samples: the sums carry their own per-pixel sample count). This text is the specification:
 *   Rounds. cfg->spp is the cap. Round 0 gives every pixel of the rectangle the samples [sample0, sample0 + min_spp): the first half is ADDED to
 *   A, the second half to B. Round r >= 1 gives every still-active pixel the next k = min(step_spp, samples left to the cap) samples, split the
 *   same way. Each half is added exactly as ptx_render adds it (in sample order), so a pixel with n samples holds, bit for bit, what ptx_render
 *   calls of the same half ranges leave in it. After each round comes one decision; the loop ends when no pixel is active or the cap is reached.
 *   Decision (IEEE binary32, every operation rounded on its own in the parenthesisation written here; max(a, b) returns the other operand when
 *   one is NaN):
 *     ma.c = a.c / a.w and mb.c = b.c / b.w for c = r, g, b;
 *     d = (|ma.r - mb.r| + |ma.g - mb.g|) + |ma.b - mb.b|;   m = ((ma.r + mb.r) + (ma.g + mb.g)) + (ma.b + mb.b);
 *     e2 = ((d * d) * 0.25f) / max(m * 0.5f, 0.01f);   noisy_p = !(e2 <= threshold * threshold) — a NaN (a zero count, a non-finite sum) is
 *     noisy: a pixel is never stopped on garbage;
 *     active_p = !done_p && (some q in the 3 x 3 block around p, clipped to the RECTANGLE, is noisy);   done_p |= !active_p.
 *   The latch means that a pixel that stopped never restarts: its samples are always a prefix [sample0, sample0 + n_p), n_p = a.w + b.w.
 *   Active list. The active pixels as tile-local indices ly * w + lx, in this order: the 32 x 32 tiles of the rectangle, row-major, anchored at
 *   the rectangle's origin; inside a tile its 8 x 8 blocks, row-major; inside a block its rows. The list is a function of the mask alone.
 * ptx_adaptive_cfg: min_spp even and >= 2; step_spp even, 0 = min_spp; threshold 0 is legal (only pixels with d == 0 stop), +inf is legal
 * (everything but NaN pixels stops after round 0).
 * ptx_adaptive_stats: render = sums over all rounds' render calls (render.samples = the sum of the per-pixel counts); rounds = rounds rendered;
 * active_last = pixels still active after the last decision (at the cap: those that would have gone on); select_ms = HIP-event time of the
 * decision kernels.
 * The two buffers are both device or both host memory; host buffers are staged once for the whole call. The call ALWAYS synchronises: once per
 * round for the 4-byte active count (with stats, once more per render call). Tile rectangles (at most 16384 x 16384) and spp_per_pass work as
 * in ptx_render, and both integrators are accepted. A rectangle is decided on its own: the 3 x 3 block is clipped to it, so along the cuts a
 * frame rendered in rectangles may stop pixels that the whole frame's decision keeps.
 * Image write: ptx_accum_mean, then ptx_tonemap_encode(..., spp = 1, ...).
 * The result is filtered by ptx_denoise_counts (ptx_denoise takes one count per buffer, not one per pixel).
 * Interleaved tile sharding (cfg->shard_count > 1): with a mask exchange registered on the scene's context the call runs the SHARDED loop
 * specified at ptx_ctx_set_mask_exchange below, and the sum of the ranks' zero-initialised half-buffers is bitwise this call's unsharded result
 * (multigpu.render_adaptive_tiles is the multi-process driver). With shard_count <= 1 a registration is ignored: the same bits, and the
 * exchange is never called.
 * Out of scope: ptx_render_transparent's blend (a recurrence, not a sum).
 * Refusals, all decided before any device work: PTX_ERR_INVALID for NULL arguments, an odd or zero min_spp, an odd step_spp, cfg->spp odd or
 * below min_spp, more than 4096 rounds, a negative or NaN threshold, pointers of mixed kinds, and whatever ptx_render refuses in cfg;
 * PTX_ERR_UNSUPPORTED for shard_count > 1 with no mask exchange registered (the 3 x 3 block reads the noisy bytes of pixels that other shards
 * own: see ptx_ctx_set_mask_exchange); PTX_ERR_INVALID for shard_count > 1 with a registered mask of fewer than w * h bytes of the rectangle, or
 * an image of more than 2^32 - 1 shard tiles; PTX_ERR_NO_DEVICE for a host-only scene. */
typedef struct ptx_adaptive_cfg { uint32_t min_spp, step_spp; float threshold; } ptx_adaptive_cfg;
typedef struct ptx_adaptive_stats { ptx_render_stats render; uint32_t rounds, active_last; double select_ms; } ptx_adaptive_stats;
int ptx_render_adaptive(ptx_scene* scene, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, float* accum_a, float* accum_b,
                        ptx_adaptive_stats* stats /* NULL ok */);
/* One decision of the specification above on the caller's buffers — the kernels ptx_render_adaptive's loop runs; for callers that drive their
 * own loop. accum_a, accum_b [h][w][4]; done [h][w] (one byte per pixel, 0 / 1) is read and updated; pixels [w * h] receives the active list
 * (NULL: none is written); the four are all device or all host memory. *n_active (host memory) receives the list's length: the call
 * synchronises. PTX_ERR_INVALID for a NULL ctx, buffer, done or n_active, w or h of 0 or above 16384, a negative or NaN threshold, pointers of
 * mixed kinds. */
int ptx_adaptive_select(ptx_ctx* ctx, uint32_t w, uint32_t h, const float* accum_a, const float* accum_b, float threshold,
                        uint8_t* done /* in/out [h][w] */, uint32_t* pixels /* out [w*h], NULL ok */, uint32_t* n_active);
/* out.c = (a.c + b.c) / (a.w + b.w) for all four channels (IEEE binary32, each operation rounded on its own); with accum_b == NULL
 * out.c = a.c / a.w. A pixel of zero count gives NaNs. out_rgba [n_pixels][4] may be accum_a or accum_b itself; all pointers device or all
 * host. PTX_ERR_INVALID for a NULL ctx, accum_a or out_rgba, n_pixels above 2^31 - 1, or pointers of mixed kinds. */
int ptx_accum_mean(ptx_ctx* ctx, const float* accum_a, const float* accum_b /* NULL ok */, size_t n_pixels, float* out_rgba);

/* ptx_render_adaptive and ptx_render_adaptive_nee over interleaved tile shards: the one thing the decision needs from the other ranks is the
 * NOISY BYTE of the pixels they own, one byte per pixel per round (2 MB at 1080p). The library does not talk to the other ranks itself: the
 * caller registers an exchange on the context, and calls with cfg->shard_count > 1 on that context's scenes run the loop below. This text is
 * the specification; everything it does not change is ptx_render_adaptive's text.
 *   Ownership. ts = shard_tile ? shard_tile : 64, tiles_x = (W + ts - 1) / ts. Rank shard_index owns the pixel (x, y) of the FULL image (the
 *   rectangle's x0, y0 added to its local coordinates) when ((y / ts) * tiles_x + x / ts) % shard_count == shard_index: the pixels ptx_render
 *   gives it under the same shard_* fields.
 *   Own pixels only. Rendering, both half-buffers and the active list cover the rank's own pixels only; other shards' pixels of accum_a and
 *   accum_b are left untouched, as in ptx_render.
 *   The mask. After a round the rank writes mask[ly * w + lx] = noisy_p (0 / 1) for its own pixels of the rectangle and 0 for all others,
 *   synchronises the context's stream, and calls fn(user, mask, w * h). On return the mask must hold, for every pixel of the rectangle, a
 *   nonzero byte iff some rank wrote a nonzero one: an element-wise MAX or OR over the ranks (a byte SUM serves for up to 255 ranks). The
 *   library reads the merged mask only as "nonzero = noisy".
 *   The decision. Every rank decides the WHOLE rectangle from the merged mask, with the `done` latch over all of its pixels, so `done`, the
 *   number of active pixels and the number of rounds are the same on every rank without a second collective. The rank's active list is the
 *   specified list order restricted to its own pixels. The loop ends when no pixel of the rectangle is active, or at the cap. A rank that owns
 *   no active pixel, or no pixel at all, renders nothing in that round and still calls the exchange: exactly one call per round on every rank.
 *   By induction over the rounds, own pixels hold what the unsharded call leaves in them and the merged mask is the unsharded call's noisy mask:
 *   the sum of the ranks' zero-initialised buffers is bitwise the unsharded result.
 * The mask buffer is the CALLER's, at least w * h bytes of the rendered rectangle, device or host memory (the library looks at the pointer): a
 * device buffer is written and read in place, so that a framework can hand its own tensor to a collective; a host buffer makes the library
 * copy its device mask out before the callback and back in after it. fn == NULL clears the registration (user, mask and mask_bytes are then
 * ignored).
 * The callback. Before it is called the library has synchronised the context's stream. It returns when the merged mask is in the buffer: it
 * has either synchronised itself, or enqueued its collective on ptx_ctx_stream(ctx), which it obtained BEFOREHAND: the callback runs under
 * the context's lock and must not call the library on that context (it would wait for itself). A non-zero return ends the render call with
 * PTX_ERR_HIP and the message "mask exchange failed (status n)"; the half-buffers then hold the completed rounds.
 * Stats of a sharded call: render.*, light_samples and light_visible are the rank's own sums; rounds is the same on all ranks; active_last is
 * the rank's own active pixels after the last decision (the sum over the ranks is the unsharded value). The sharded loop synchronises twice per
 * round: before the callback, and for the 8 bytes of the two counts.
 * ptx_ctx_get_mask_exchange_stats: the number of callback calls of the context's last adaptive call (0 after an unsharded one) and the wall
 * time spent inside them; either pointer may be NULL.
 * PTX_ERR_INVALID for a NULL ctx, and for a callback with a NULL mask. Out of scope: a library-owned RCCL path for the mask, and
 * ptx_adaptive_select with shards. */
typedef int (*ptx_mask_exchange_fn)(void* user, uint8_t* mask, size_t n_bytes);
int ptx_ctx_set_mask_exchange(ptx_ctx* ctx, ptx_mask_exchange_fn fn /* NULL clears */, void* user, uint8_t* mask, size_t mask_bytes);
int ptx_ctx_get_mask_exchange_stats(ptx_ctx* ctx, uint64_t* calls /* NULL ok */, double* wall_ms /* NULL ok */);

/* Next-event estimation towards emissive triangles (no counterpart in the reference, whose estimators collect emission only where a
 * BSDF-sampled ray happens to hit an emitter). ptx_render_nee renders the samples of ptx_render with the PTX_INTEGRATOR_LIB estimator plus
 * one light sample per continuing vertex: same cfg fields, Philox keys and camera rays, sums in ptx_render's accum format, alpha + 1 per
 * sample. The light sample is combined with the BSDF-sampled emission by the balance heuristic so that ITS EXPECTATION IS LIB'S.
 * LIB's clamp T *= clamp(brdf / max(pdf, eps), 0, 1) means LIB integrates brdf' = qc * pe with pe = max(pdf, eps) and
 * qc = clamp(brdf / pe, 0, 1) per channel; the light sample uses the same brdf' and introduces no other clamp.
 * A vertex runs LIB's rules exactly as ptx_render has them (miss and environment, opacity pass-through with pass + 1 and the 4096 bound,
 * back face, sun request, shadow catcher pending then pass-through, last vertex, T update, depth++, pass = 0). Two things change:
 *   EMISSION WEIGHT. L += (T * emissive10) * w. w = 1 (no arithmetic) when depth == 0, or pass > 0 (the ray came through a surface: no
 *     light sample can produce that path), or the hit triangle is not listed. Otherwise w = p_prev / (p_prev + p_l) with
 *     p_l = (dist * dist) / (cg * A_total), cg = |dot(ng, d)|, ng the listed triangle's geometric normal, dist the hit distance and
 *     p_prev the pe of the direction sampled at the previous vertex.
 *   LIGHT SAMPLE, at every vertex that reaches LIB's BSDF sample, before it and whatever its outcome (a last vertex takes none; none at
 *     all when the list is empty): r = draws(pixel, sample, depth, pass, block 3); triangle i = the first with r.x < cdf[i] (index clamped
 *     to n - 1); su = sqrt(r.y), beta = su * (1 - r.z), gamma = su * r.z; position pos_y, shading normal n_y and Le = 10 * emissive(uv) of
 *     the point (beta, gamma) of triangle i, as a hit there would give them; v = pos_y - pos_x, dist2 = dot(v, v), w = v / sqrt(dist2).
 *     No contribution and no shadow ray unless dist2 > 0, dot(n_x, w) > 0, dot(n_y, -w) > 0, cg = |dot(ng_i, w)| > 0 and max(Le) > 0.
 *     brdf, pdf = LIB's BSDF value for w with the vertex's own specular probability and roughness; pe = max(pdf, eps),
 *     qc = clamp(brdf / pe, 0, 1), p_l = dist2 / (cg * A_total), wl = pe / (pe + p_l); x = ((T * qc) * wl) * Le with T before its update.
 *     The shadow ray (origin pos_x + w * eps, direction w) is a CLOSEST-hit query on the scene's route; x is added iff that hit is
 *     triangle i of that surface (identity, no distance epsilon).
 * Order of the additions of one sample, fixed and without float atomics: vertex k's emission, its sun term if unoccluded, its light term
 * if visible, then vertex k + 1. With an empty list every w is exactly 1 and no light term exists: the frame is bitwise ptx_render's.
 * THE LIGHT LIST (PTX_ARR_LIGHT_*): a surface is listed iff its emissive factor has a positive component, it cannot pass a sample
 * through (constant opacity approximately 1, no texture feeding opacity) and it is not a shadow catcher; unlisted emitters keep w = 1, so
 * nothing is lost or counted twice. Per listed surface in surface order and triangle in mesh order, in float64: world corners, area =
 * |e1 x e2| / 2 (a triangle whose area is not > 0 is left out), ng = normalize(e1 x e2), running sum; stored as float32.
 * Tiles, sample0, spp_per_pass, shard_*, host or device accum and bounces == 0 work as in ptx_render.
 * Refusals, all decided before any device work: PTX_ERR_UNSUPPORTED for PTX_INTEGRATOR_WORKER; PTX_ERR_NO_DEVICE for a host-only scene;
 * PTX_ERR_INVALID for NULL scene, cfg or accum, unknown flags and whatever ptx_render refuses in cfg.
 * ptx_render_adaptive_nee (below the flags) runs ptx_render_adaptive's loop on this estimator.
 * Out of scope: ptx_render_transparent's blend and the worker estimator. multigpu.py needs no function of its own for this call: its shards
 * and sample ranges already compose through the accum format. */
#define PTX_NEE_NO_LIGHT_SAMPLES 1u   /* run with an empty list */
/* PTX_NEE_FUSED: render with ONE kernel launch per pass wherever ptx_render would run this scene on its fused kernel (pipeline 0: LDS-resident and
 * hybrid scenes, global-memory scenes under PTX_WAVEFRONT=0): a lane carries a path from its camera ray to its end in registers, without the
 * per-round host synchronisation and the 68 words of stream workspace per sample of the default form. The estimator above is the specification
 * of both forms, order of the additions included: for every cfg, accum is bit for bit what the unflagged call leaves, and rays, samples,
 * n_lights, light_area, light_samples and light_visible of the stats are equal. render.passes = the launches (the pass size and id limit are
 * ptx_render's, since the only per-sample workspace is the 16-byte radiance record), render.kernel_ms = their event time; ptx_ctx_get_timing
 * then reports pipeline 0, fused_launches == passes and fused_ms == kernel_ms. On a scene of the queue route (pipeline 1) the flag is ignored
 * and the call runs exactly as without it (fused_launches == 0) — not a refusal, so a caller may always set it. May be combined with
 * PTX_NEE_NO_LIGHT_SAMPLES. Value 2u is unassigned and refused as unknown. */
#define PTX_NEE_FUSED 4u
/* PTX_NEE_ENV_SAMPLES: the light sample of a vertex may go towards the environment map (ptx_scene_set_environment), importance-sampled by
 * luminance; the map's radiance collected on a miss is weighted against that sample, so the expectation of the frame is still LIB's
 * (as far as LIB's pdf is the density of LIB's sampler, which its specular lobe's is not: DESIGN.md 5.7 has the measured shift, PTX_NEE_SAMPLER_PDF below removes it).
 * Ignored when the scene has no map or the map is black: the call is then bit for bit the one without the flag. Combines with
 * PTX_NEE_FUSED (bitwise the same frame; ignored on the queue route as above) and with PTX_NEE_NO_LIGHT_SAMPLES, which empties the
 * triangle list only. Values 2u, 8u and 32u are unassigned and refused as unknown.
 *   THE ENVIRONMENT TABLE (PTX_ARR_ENV_*), for a map of w x h texels, built on the host in float64 and stored as float32. Box (i, j) is
 *     u in [i / w, (i + 1) / w), 1 - v in [j / h, (j + 1) / h) of the miss lookup u = atan2f(d.z, d.x) * 0.1591F + 0.5F,
 *     v = asinf(d.y) * 0.3183F + 0.5F. lum(i, j) = 0.2126 r + 0.7152 g + 0.0722 b of the texel as the kernels read it (sRGB table, missing
 *     channels 1), a negative or NaN luminance counting as 0. weight(i, j) = (sum of lum over the 3 x 3 texels around (i, j), wrapped modulo
 *     w and h as the bilinear lookup wraps: every texel the lookup can touch from inside the box) * max(cos(lat_j), 0) with
 *     lat_j = ((1 - (j + 0.5) / h) - 0.5) / 0.3183. row_cdf[j] = cumulative row mass / total, cell_cdf[j][i] = cumulative weight of row j /
 *     its mass, last entries 1, a row of zero mass all 0. Total mass 0: no table.
 *   THE PDF env_pdf(d), a function of the direction alone, used by both sides: (u, v) by the lookup's expressions; i = min((uint32_t)(u * w),
 *     w - 1), j likewise from (1 - v) * h; P = (row_cdf[j] - row_cdf[j - 1]) * (cell_cdf[j][i] - cell_cdf[j][i - 1]) from the stored values
 *     with cdf[-1] = 0; c = sqrt(max(0, 1 - d.y * d.y)); env_pdf = ((P * (float)(w * h)) * (0.1591F * 0.3183F)) / c, and 0 when c is not
 *     > 0. P from the stored differences is exactly what the sampler realises: a box that float32 rounds to probability 0 is never sampled
 *     and has weight 1 on the BSDF side.
 *   SELECTION. c_env = 1 when the triangle list is empty, 0.5 when both strategies exist. With r = draws(.., block 3) the vertex samples the
 *     map iff the list is empty or r.w < 0.5F; otherwise a triangle as above. Wherever the formulas above have p_l, (1 - c_env) * p_l
 *     takes its place (the emission weight and wl).
 *   ENVIRONMENT SAMPLE: q = draws(pixel, sample, depth, pass, block 4); row j = the first with q.x < row_cdf[j] (clamped to h - 1), column
 *     i = the first with q.y < cell_cdf[j][i] (clamped to w - 1); u = (i + q.z) / w, v = 1 - (j + q.w) / h; phi = (u - 0.5F) / 0.1591F,
 *     lat = (v - 0.5F) / 0.3183F; w_dir = (cos lat * cos phi, sin lat, cos lat * sin phi). No contribution and no shadow ray unless the
 *     lookup maps w_dir to box (i, j) again (this drops the sliver of (u, v), about 3e-4 of the domain, that the truncated constants make
 *     unreachable for the lookup, and keeps the pdf a function of direction), dot(n_x, w_dir) > 0, p = env_pdf(w_dir) > 0 and max(Le) > 0
 *     with Le = lookup(w_dir).rgb * cfg.env. brdf, pe, qc as for a triangle sample; wl = pe / (pe + c_env * p); x = ((T * qc) * wl) * Le.
 *     The shadow ray (origin pos_x + w_dir * eps, direction w_dir) is a closest-hit query; x is added iff it finds nothing.
 *   MISS WEIGHT. L += (T * env) * wm. wm = 1 (no arithmetic) when depth == 0 or pass > 0; otherwise wm = p_prev / (p_prev + c_env * env_pdf(d)).
 * Order of the additions and the stats are unchanged: light_samples and light_visible count both kinds of light ray. */
#define PTX_NEE_ENV_SAMPLES 16u
/* PTX_NEE_SAMPLER_PDF: the MIS weights are built on the density of LIB's BSDF SAMPLER instead of pe, LIB's pdf VALUE. The two differ in the
 * specular lobe: importance_ggx draws a half vector h with cos_theta = sqrt((1 - u) / (1 + (a2 - 1) u)), a2 = roughness^4, a uniform azimuth,
 * and returns reflect(-o, h), so the density of its direction w is D(h) (n.h) / (4 (o.h)) with D = a2 / (pi ((n.h)^2 (a2 - 1) + 1)^2), which
 * LIB's pdf_specular is not (E[cos / pdf_specular] over the sampler's directions is 2.9 to 62 where pi is expected). The
 * diffuse draw is exactly cosine-weighted, so pdf_diffuse is its density. With weights on pe the two techniques do not sum to LIB's integrand
 * wherever a glossy vertex sees a light; with this flag they do, and the expectation of the frame is LIB's.
 *   THE DENSITY ps(w) of a vertex, from its own normal, outcoming, spec_prob and the roughness importance_sample receives (after
 *     max(roughness, 0.05F)), IEEE binary32, each operation rounded on its own:
 *       a = roughness * roughness;  a2 = a * a
 *       hv = outcoming + w;  h = hv / sqrt(dot(hv, hv))
 *       nh = dot(normal, h);  oh = dot(outcoming, h)
 *       t = (nh * nh) * (a2 - 1) + 1
 *       ps_spec = (nh > 0 && oh > 0) ? (a2 * nh) / ((((float)pi * t) * t) * (4 * oh)) : 0
 *       ps_diff = pdf_diffuse(normal, w), the value eval_brdf uses
 *       ps = lerpf(ps_diff, ps_spec, spec_prob), the mixture the draw rnd.y < spec_prob realises
 *   ps takes pe's place in the weights and only there:
 *     p_prev = ps(inc) after the BSDF sample; if that is not a positive finite number, p_prev = pe as without the flag.
 *     wl = ps / (ps + p_l') for the triangle sample and for the environment sample, p_l' being p_l, (1 - c_env) * p_l or c_env * p as above.
 *     A light sample with !(ps > 0) contributes nothing and traces no shadow ray (and is not counted in light_samples).
 *     qc, the T update, the sun term, the draws, their Philox blocks and the order of the additions are unchanged; the emission weight and
 *     the miss weight keep their formulas and read the new p_prev.
 *   The sum of the two techniques is then the integral of ps * qc * Le, which is what LIB's vertex integrates.
 * Combines with PTX_NEE_FUSED (bitwise the same frame; ignored on the queue route as above), with PTX_NEE_ENV_SAMPLES and with
 * PTX_NEE_NO_LIGHT_SAMPLES; ptx_render_adaptive_nee passes it through. With no light sample possible (empty list and no environment table)
 * every weight is exactly 1 and the call is bit for bit the one without the flag. Without the flag nothing changes. */
#define PTX_NEE_SAMPLER_PDF 64u
/* PTX_NEE_CANDIDATES(m), m = 1 .. 16: the light sample of a vertex is picked among M = m candidates in proportion to their unshadowed
 * contributions (resampled importance sampling), and ONE shadow ray is traced for it. The count travels in bits 8..11 of flags:
 * M = ((flags >> 8) & 15) + 1, so PTX_NEE_CANDIDATES(1) is 0, the call without it. 8192 is PTX_NEE_FUSED_MOTION (below); 4096, the bits at
 * 16384 and above, and the values 2, 8, 32 and 128 stay unassigned and refused as unknown. The estimator for M > 1 is the text of ptx_render_nee above with the LIGHT SAMPLE paragraph
 * replaced by the following; IEEE binary32, each operation rounded on its own, in the order written.
 *   CANDIDATES. Candidate j = 0 .. M - 1 is the light sample of the call without these bits, taken verbatim (with PTX_NEE_ENV_SAMPLES its
 *     SELECTION and ENVIRONMENT SAMPLE, with PTX_NEE_SAMPLER_PDF its ps), with Philox block 3 + 2 j in the place of block 3 and block
 *     4 + 2 j in the place of block 4: candidate 0 is that call's sample. A candidate that there contributes nothing and traces no shadow
 *     ray is dropped. A surviving one yields its x_j, its shadow ray and its visibility rule (the closest hit is triangle i of that surface,
 *     or: the ray hits nothing).
 *   WEIGHT AND SELECTION. W_j = max(x_j.r, x_j.g, x_j.b); a candidate whose W_j is not a positive finite number is dropped. For every kept
 *     candidate, in the order of j: wsum = wsum + W_j; u_j = component j & 3 of draws(pixel, sample, depth, pass, block 0x100 + (j >> 2));
 *     the first kept candidate is chosen outright, a later one replaces the choice iff u_j * wsum < W_j.
 *   ESTIMATE. No kept candidate: no light ray. Otherwise, for the chosen y, x = x_y * ((wsum / (float)M) / W_y), with y's shadow ray and
 *     visibility rule. M counts all candidates, the dropped ones included.
 * Nothing else changes: the emission weight, the miss weight, p_prev, qc, the T update, the sun term, the order of the additions and the
 * draws of every other block. In particular p_l and env_pdf in the BSDF-side weights stay the densities of a SINGLE candidate.
 * light_samples and light_visible count the light rays traced: at most one per vertex.
 * The expectation is still LIB's. Every x_j is already F(y_j) / p(y_j), with F the MIS-weighted integrand of the light side and p the
 * density of one candidate (the mixture over triangles and map, selection probability included). Resampling with the target
 * W = max(F) / p is unbiased for the integral of F: E[(F(y) / max(F(y))) * (1 / M) sum_j W_j * V(y)] = integral of F V. The light-side and
 * the BSDF-side weights are functions of the direction alone that still add to one, so the two sides together integrate LIB's vertex.
 * What falls is the variance (DESIGN.md 5.7 has the measurement), at the price of M - 1 further candidates' arithmetic and no further ray.
 * Combines with every other flag; ptx_render_adaptive_nee passes the bits through. With PTX_NEE_FUSED the frame and the stats equal the
 * unfused call's with the same bits (on the queue route PTX_NEE_FUSED is ignored as above). With no light sample possible (empty list and
 * no environment table) no candidate is drawn, and the call is bit for bit the one without the bits, and ptx_render. */
#define PTX_NEE_CANDIDATES(m) ((((uint32_t)(m)) - 1u) << 8)   /* m = 1 .. 16; m = 1 is 0: today's call */
/* PTX_NEE_FUSED_MOTION: lets PTX_NEE_FUSED hold under active motion (ptx_scene_set_motion: MOTION above). With both bits, on a scene of the
 * fused route (pipeline 0) whose motion is active, the call runs ONE launch per pass of the fused kernel that carries a time per lane.
 * accum is bit for bit what the unflagged call leaves under the same motion, and rays, samples, n_lights, light_area, light_samples and
 * light_visible are equal; render.passes = the launches, with ptx_render's pass size and id limit as for PTX_NEE_FUSED, and
 * ptx_ctx_get_timing reports pipeline 0, fused_launches == passes and fused_ms == kernel_ms. Instead of the 68 (under motion up to 71)
 * words of stream workspace per sample and one host synchronisation per round, the call needs the 16-byte radiance record per sample.
 *   Without PTX_NEE_FUSED the bit is accepted and does nothing. With PTX_NEE_FUSED but no active motion (never set, all keys equal, or
 *   cleared) the call is the PTX_NEE_FUSED call: the same kernels, bits and fused_launches. On the queue route it is ignored as
 *   PTX_NEE_FUSED is (fused_launches == 0). PTX_NEE_FUSED alone under active motion stays ignored: a caller opts in to the motion kernel.
 *   With a non-empty light list in tree mode (ptx_scene_set_light_pick, LIGHT PICK below) under active motion both bits together are
 *   ignored in the same way (fused_launches == 0): the motion kernel has no tree variants, and the unfused form runs the tree.
 * Combines with every other flag and with PTX_NEE_CANDIDATES(m); ptx_render_adaptive_nee passes it through, and its rounds then run fused
 * launches. The light-list rule (a surface of a moving model is not listed) and every refusal under active motion are unchanged.
 * PTX_NEE_NO_LIGHT_SAMPLES | PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION is ptx_render's estimator under a shutter in one launch per pass.
 * The kernel holds more state per lane than its static twin (the time, the blended basis of a moving ray space, a moving surface's
 * records), and some variants run at a smaller workgroup for it: DESIGN.md 5.12 has the register table and the measurement. */
#define PTX_NEE_FUSED_MOTION 8192u
/* PUNCTUAL LIGHTS. With punctual lights on the scene (ptx_scene_set_punctual_lights) ptx_render_nee and ptx_render_adaptive_nee take them into
 * the LIGHT SAMPLE of a vertex as a third strategy. No flag exists for it: a scene on which none were set (or on which they were cleared) runs
 * the kernels without the branch and renders every bit as before. ptx_render, ptx_render_transparent, ptx_render_aov and the WORKER estimator
 * ignore the lights. IEEE binary32, each operation rounded on its own, in the order written.
 *   SELECTION. "Other strategies exist" means: the triangle list is non-empty, or PTX_NEE_ENV_SAMPLES is set and a table exists. c_p = 1 when
 *     no other strategy exists, else 0.5. Candidate j draws q = draws(pixel, sample, depth, pass, block 0x200 + j); the call without
 *     PTX_NEE_CANDIDATES is j = 0. Candidate j is a punctual sample iff c_p == 1 or q.x < 0.5F; otherwise it is the candidate of the text
 *     above, from its blocks 3 + 2 j and 4 + 2 j, unchanged. Light k is the first entry with q.y < cdf[k], the index clamped to n - 1.
 *   PUNCTUAL SAMPLE. v = position_k - pos_x, dist2 = dot(v, v), dist = sqrt(dist2), w = v / dist. att = 1 for a point light; for a spot
 *     cd = dot(direction_k, -w), s = clamp((cd - cos_outer) / max(cos_inner - cos_outer, 1e-6F), 0, 1), att = s * s.
 *     E = (intensity_k * att) / dist2. No contribution and no shadow ray unless dist2 > 0, dot(n_x, w) > 0, pmf_k > 0,
 *     range == 0 || dist <= range, att > 0 and max(E) > 0. brdf, pdf, pe and qc are those of a triangle sample; b = qc * pe, LIB's integrand
 *     brdf' at w, cosine included (eval_brdf carries it); x = ((T * b) * E) / (c_p * pmf_k) with T before its update. A delta light has no
 *     MIS partner: its weight is 1, and PTX_NEE_SAMPLER_PDF changes nothing in this sample. The shadow ray (origin pos_x + w * eps,
 *     direction w) is a closest-hit query on the scene's route; x is added iff it finds nothing or its hit distance t is not < dist. A
 *     surface of opacity < 1 in the way blocks the light, as it blocks a triangle sample.
 *   THE OTHER WEIGHTS. The other strategies take only 1 - c_p of the candidates. CONVENTION: wherever the text above has a light-side density
 *     in a weight — p_l, (1 - c_env) * p_l or c_env * p in wl, in the emission weight and in the miss weight — that density is first computed
 *     exactly as written there, its c_env factor included, and the result is then multiplied from the left: p' = (1 - c_p) * p. With c_p == 1
 *     no other strategy exists and none of these weights is evaluated.
 *   CANDIDATES. Under PTX_NEE_CANDIDATES(m) a punctual candidate is one more kind of candidate: the same W_j = max(x_j), the same reservoir,
 *     one shadow ray for the pick, with the punctual visibility rule when the pick is punctual. PTX_NEE_NO_LIGHT_SAMPLES empties the triangle
 *     list only. light_samples and light_visible count punctual rays like the others; the order of the additions of a sample is unchanged.
 *   EXPECTATION. A punctual candidate has selection probability c_p * pmf_k and returns brdf'(w_k) E_k V_k over it: unbiased for the sum over
 *     the lights. The other strategies' light-side and BSDF-side weights still add to one over the directions they share.
 * PUNCTUAL PICK (ptx_scene_set_punctual_pick, PTX_PUNCTUAL_PICK_TREE). The CDF above picks a lamp across the room as often as the lamp
 * overhead. In tree mode two things change in the text above and nothing else: which light k a punctual candidate samples, and the pmf that
 * stands wherever the text has pmf_k. A delta light has no MIS partner, so no other weight knows the pick: c_p, the (1 - c_p) convention,
 * the reservoir, the visibility rule, the counters and the order of the additions are as written, and so is the condition pmf_k > 0. No NEE
 * flag exists for it and no variant: the PUN kernels test one kernel argument, uniform over the launch.
 *   THE TREE (PTX_ARR_PUNCTUAL_TREE), built on the host, deterministic. Leaves are the stored lights with lum_k > 0, lum_k =
 *     (0.2126 r + 0.7152 g) + 0.0722 b of the float32 intensity in float64; a black light is in no leaf. A node is 8 words: lo.xyz (0-2) and
 *     hi.xyz (4-6), the float32 bounds of the positions below it; power (3), the float64 sum of the lum_k below it in the node's light order,
 *     stored as float32; word 7 = 0x80000000 | light index for a leaf, for a branch the index of its left child, whose right sibling is the
 *     next node. The root is node 0 over the lights in index order. Nodes are split in FIFO order. A node over one light is a leaf. Otherwise
 *     the axis is the largest extent hi - lo, taken in float64 from the float32 values, the lowest axis winning a tie; the lights are sorted
 *     by (position[axis], index); the first count / 2 (integer division) go left, in that order, the others right; the two children take
 *     the next two free slots, left first. m leaves give 2 m - 1 nodes and a depth of at most ceil(log2 m) + 1; the trip counts of two
 *     descents differ by one at most.
 *   THE IMPORTANCE of child N seen from x. IEEE binary32, each operation rounded on its own, in the order written; dot is the device's,
 *     (a.x b.x + a.y b.y) + a.z b.z. Branch: c = (lo + hi) * 0.5F, d = x - c, h = (hi - lo) * 0.5F, I = power / max(dot(d, d), dot(h, h)):
 *     inside the box's sphere the distance says nothing, and the node counts with its half diagonal. Leaf of light k: v, dist2, dist, w, att
 *     and the range test are the expressions of PUNCTUAL SAMPLE (one device function shared with the sample); I = (power * att) / dist2
 *     when dist2 > 0 and the light is in range, else 0. So a leaf's importance is exactly 0 precisely where the sample's own geometric
 *     conditions fail, and the cone of a spot steers the last step of the descent.
 *   THE PICK, with u = q.y of the candidate's block 0x200 + j, node = 0, pmf = 1. While node is a branch with children l and l + 1:
 *     s = I_l + I_r; p = I_l / s, or 0.5F if s is not a positive finite number. If u < p: pmf = pmf * p, u = u / p, go left. Otherwise
 *     q1 = 1 - p, pmf = pmf * q1, u = (u - p) / q1, go right. Then u = min(u, 0x1.fffffep-1F). The leaf's light is k and pmf is pmf_k. A
 *     light whose realised pmf rounds to 0 from some point is not sampled from there, as under the CDF. With one light the root is its leaf:
 *     (0, 1.0F), and the frame is the CDF mode's bit for bit.
 *   EXPECTATION. The pmf is a function of x alone and positive wherever E_k(x) > 0 (a leaf with I > 0 has p > 0 at every branch above it),
 *     so the punctual term stays unbiased for the sum over the lights. What falls is the variance; DESIGN.md 5.13 has the measurement.
 *   Out of scope: emissive triangles in the tree (their MIS weights need the pick's density from the previous vertex), orientation and cone
 *     bounds in the branches, the receiver's cosine, a tree for the environment map, lights that move under a shutter.
 * LIGHT PICK (ptx_scene_set_light_pick, PTX_LIGHT_PICK_TREE). The CDF over area picks a small emitter across the scene as often as an equal
 * one a hand's breadth away. In tree mode with a non-empty list exactly three things change in the text of ptx_render_nee: the LIGHT
 * SAMPLE's triangle and density, the EMISSION WEIGHT's density, and the path state, which gains x_prev. ENV, SPDF, RIS, PUN, the draws, the
 * blocks, the visibility rule, the counters and the order of the additions stay as they are. With an empty list (or
 * PTX_NEE_NO_LIGHT_SAMPLES) the mode is ignored bit for bit. IEEE binary32, each operation rounded on its own, in the order written.
 *   THE TREE (PTX_ARR_LIGHT_TREE, PTX_ARR_LIGHT_PATH), built on the host with the light list, deterministic. The leaves are the entries
 *     of the list, in list order. Per entry, in float64 from the float64 world corners c0, c1, c2 of THE LIGHT LIST: centroid =
 *     ((c0 + c1) + c2) / 3; the box of the three corners; power_k = area_k * lum, lum = (0.2126 r + 0.7152 g) + 0.0722 b of the float32
 *     emissive factor. Every listed surface has a positive component, so every leaf's power is positive. The emissive TEXTURE is not
 *     consulted. A node is 8 words: lo.xyz (0-2) and hi.xyz (4-6), the float32 bounds of the CORNERS below it (each corner coordinate
 *     rounded to float32, then the minimum and maximum); power (3), the float64 sum in the node's entry order, stored as float32; word 7 =
 *     0x80000000 | list entry for a leaf, for a branch the index of its left child, whose right sibling is the next node. The root is node
 *     0 over the entries in list order. Nodes are split in FIFO order. A node over one entry is a leaf. Otherwise the axis is the largest
 *     extent of the bounds of the float64 centroids below it, the lowest axis winning a tie; the entries are sorted by (centroid[axis],
 *     index); the first count / 2 (integer division) go left, in that order, the others right; the two children take the next two free
 *     slots, left first. m entries give 2 m - 1 nodes and a depth of at most ceil(log2 m) + 1. Bit i of path[k] is 1 iff step i of the
 *     descent from the root to leaf k goes right. A list of more than 2^30 entries is refused in tree mode at the render
 *     (PTX_ERR_UNSUPPORTED).
 *   THE IMPORTANCE of node N seen from x, ONE formula for leaves and branches: c = (lo + hi) * 0.5F, d = x - c, h = (hi - lo) * 0.5F,
 *     I = power / max(dot(d, d), dot(h, h)), dot the device's (a.x b.x + a.y b.y) + a.z b.z. I is positive everywhere, so every listed
 *     triangle has a positive pmf wherever the product is finite and does not underflow. There is no orientation term: the sample's own
 *     conditions (dot(n_y, -w) > 0, cg > 0) may reject a picked triangle, which costs variance, not expectation.
 *   THE PICK from x with draw u is PUNCTUAL PICK's loop, word for word: node = 0, pmf = 1; while node is a branch with children l and
 *     l + 1: s = I_l + I_r; p = I_l / s, or 0.5F if s is not a positive finite number. If u < p: pmf = pmf * p, u = u / p, go left.
 *     Otherwise q1 = 1 - p, pmf = pmf * q1, u = (u - p) / q1, go right. Then u = min(u, 0x1.fffffep-1F). The leaf's entry is i.
 *   THE DIRECTED PMF pmf_k(x) is the same loop from the root, taking at step j the side that bit j of path[k] names and multiplying the
 *     same p or q1 = 1 - p in the same order (one device function gives p to both): bit for bit the pmf THE PICK returns whenever it
 *     returns k.
 *   LIGHT SAMPLE. Triangle i and pmf_i come from THE PICK at pos_x with u = r.x of the candidate's light block, instead of the CDF. No
 *     contribution unless additionally pmf_i > 0. p_l = (pmf_i * dist2) / (cg * A_i), A_i the stored float32 area geom[i].w; this replaces
 *     dist2 / (cg * A_total). The (1 - c_env) and (1 - c_p) factors then apply from the left, as the conventions say.
 *   EMISSION WEIGHT. For a listed hit triangle k at depth != 0 && pass == 0: p_l = (pmf_k(x_prev) * (dist * dist)) / (cg * A_k), then the
 *     same factors. x_prev is the pos_x of the vertex that drew the BSDF sample. If p_l == 0, w is 1 as the formula gives it: the light
 *     side never samples the triangle from there.
 *   PATH STATE. x_prev joins the path state and is set where p_prev is set (a pass-through vertex leaves both alone).
 *   CANDIDATES. Under PTX_NEE_CANDIDATES every candidate descends with its own r.x. The BSDF-side p_l stays a single candidate's density.
 *   ONE TRIANGLE. The root is a leaf and pmf = 1.0F; 1 * dist2 and A_0 == A_total are exact, so the frame is bitwise the CDF mode's.
 *   FORMS. Both forms run the tree, in variants of their own (a fourth part bit of the variant mask, NEE_LTREE): the unfused form carries
 *     x_prev in three more stream words per path, allocated and touched in tree mode only; the fused form in three registers per lane, in
 *     the tree variants only. With PTX_NEE_FUSED the frame and the stats equal the unfused call's, as in CDF mode. No kernel of the CDF
 *     mode changes (DESIGN.md 5.14 has the register table of the tree variants). Under ACTIVE MOTION the fused motion kernel is not
 *     extended: with a non-empty list in tree mode PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION is ignored as PTX_NEE_FUSED alone is
 *     (fused_launches == 0), and the unfused form runs the tree. With an empty list, PTX_NEE_NO_LIGHT_SAMPLES or CDF mode the flags act
 *     as before.
 *   EXPECTATION. pmf_i(x) is a function of x alone, positive for every listed triangle; the light-side density p_l is the true density of
 *     the direction, and the BSDF-side weight evaluates the same function at the same x: the two weights add to one over the shared
 *     directions, and the estimator's expectation is the CDF mode's.
 *   Out of scope: orientation or normal cones in the nodes; the receiver's cosine in the importance; textured emission in the power; the
 *     tree inside k_nee_fused_motion; emitters on moving models (unlisted, as before); a tree over the environment map. */
typedef struct ptx_nee_cfg { uint32_t flags; } ptx_nee_cfg;
typedef struct ptx_nee_stats {
	ptx_render_stats render;   /* rays = closest-hit + shadow queries */
	uint32_t n_lights;         /* listed triangles */
	float light_area;          /* A_total */
	uint64_t light_samples, light_visible;   /* light shadow rays traced, and how many found their triangle */
} ptx_nee_stats;
int ptx_render_nee(ptx_scene* scene, const ptx_render_cfg* cfg, const ptx_nee_cfg* ncfg /* NULL = defaults */, float* accum_rgba,
                   ptx_nee_stats* stats /* NULL ok */);

/* Noise-driven per-pixel sample counts on the light-sampling estimator: the specification is ptx_render_adaptive's text (rounds, decision,
 * latch, active list, clipping to the rectangle; the same decision kernels) with "ptx_render" read as "ptx_render_nee with ncfg->flags". After
 * the call a pixel with n samples holds, bit for bit, what ptx_render_nee calls of the same half ranges with the same flags leave in A and
 * in B — for every flag combination, on every route and for any spp_per_pass.
 * One sequence of passes per round, not two: a round's k samples [s, s + k) are planned as ptx_render_nee plans a call of spp = k on the
 * round's pixels (each form with its own default pass size and id limit), and every pass is resolved into BOTH halves: the round's samples
 * below s + k / 2 are added to A and the others to B, each in sample order. A sample's radiance is keyed by (pixel, sample) and each buffer
 * receives its samples in ascending order, so the result is bitwise that of two calls per round at half the launches.
 * Stats: nee.render and light_samples / light_visible are sums over the rounds (render.samples = the sum of the per-pixel counts,
 * render.passes = the passes launched: with the default pass size on a small frame passes == rounds); n_lights and light_area as in
 * ptx_render_nee; rounds, active_last, select_ms as in ptx_adaptive_stats. ptx_ctx_get_timing after a call with stats reports the pipeline;
 * when the fused form ran, fused_launches == nee.render.passes and fused_ms == nee.render.kernel_ms, otherwise fused_launches == 0.
 * Host buffers are staged once for the whole call; the light list and the environment table are uploaded once. The call always synchronises,
 * as ptx_render_adaptive does. Filter the result with ptx_denoise_counts; image write as for ptx_render_adaptive.
 * shard_count > 1 runs the sharded loop of ptx_ctx_set_mask_exchange, as in ptx_render_adaptive.
 * Refusals, all decided before any device work: everything ptx_render_adaptive refuses (PTX_ERR_UNSUPPORTED for shard_count > 1 without a
 * registered mask exchange) and
 * everything ptx_render_nee refuses (PTX_ERR_INVALID for an unknown flag, PTX_ERR_UNSUPPORTED for PTX_INTEGRATOR_WORKER, PTX_ERR_NO_DEVICE for
 * a host-only scene). */
typedef struct ptx_adaptive_nee_stats { ptx_nee_stats nee; uint32_t rounds, active_last; double select_ms; } ptx_adaptive_nee_stats;
int ptx_render_adaptive_nee(ptx_scene* scene, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, const ptx_nee_cfg* ncfg /* NULL = defaults */,
                            float* accum_a, float* accum_b, ptx_adaptive_nee_stats* stats /* NULL ok */);

/* Measurement aid (no counterpart in the reference): where the time of the last ptx_render that was given a stats pointer went.
 * Scenes whose geometry fits the LDS or whose models have few surfaces run ONE fused kernel per pass (pipeline 0: fused_ms);
 * many-surface scenes in global memory run the queue-based pipeline (pipeline 1) — per step of a slab of paths a classify, a
 * traverse and a shade kernel. Their HIP-event times are collected only after ptx_ctx_set_timing(ctx, 1) (four event records per
 * step); the workspace figures are always filled. */
typedef struct ptx_kernel_timing {
	uint32_t pipeline;          /* 0 = fused kernel, 1 = queue-based pipeline */
	uint32_t steps;             /* queue-based pipeline: steps timed (classify + traverse + shade each) */
	double classify_ms, traverse_ms, shade_ms;   /* sums over those steps */
	double fused_ms;            /* fused kernel: sum over its launches */
	uint32_t fused_launches;
	uint32_t pool_overflows;    /* queue-based pipeline: slabs that were repeated smaller because a step's pairs did not fit the pool */
	uint64_t pool_pairs;        /* queue-based pipeline: pairs (ray, entered surface) the pool holds, 48 bytes each */
	uint64_t peak_pairs;        /* ... the most pairs one step of one slab asked for */
	uint64_t slab_paths;        /* ... camera paths per slab */
	uint64_t workspace_bytes;   /* device memory the pipeline that ran holds on the context (streams, pool, queues) */
	double traverse_drain_frac; /* queue-based pipeline, with timing on: share of the traverse launches' wave-time between a wave running out of work
	                             * and the launch's last wave ending (the persistent waves' own clocks; 0 when not measured) */
} ptx_kernel_timing;
int ptx_ctx_set_timing(ptx_ctx* ctx, int on);
int ptx_ctx_get_timing(ptx_ctx* ctx, ptx_kernel_timing* out);

/* Batch form of renderer::intersect (renderer.cpp:645-725) / distributed_scene::intersect
 * (src/scene/scene.hpp:20-21): the unit the host's INTERSECT stage queue would call.
 * Rays are SoA; directions are used as given (the reference normalises on construction, ray.cpp:6-8,
 * so pass unit vectors). All pointers device or host (all of one kind). */
typedef struct ptx_rays {
	const float *ox, *oy, *oz, *dx, *dy, *dz;
} ptx_rays;
typedef struct ptx_hits {
	float* distance;    /* world-space hit distance; -1 = miss (model::intersection::distance, model.hpp:21) */
	int32_t* surface;   /* global surface (primitive) id, -1 = miss */
	int32_t* triangle;  /* triangle index within the surface's mesh */
	float *b0, *b1, *b2;            /* barycentrics (alpha, beta, gamma) — triangle.cpp:185-189 */
	float *px, *py, *pz;            /* world position        (may be NULL as a group of three) */
	float *nx, *ny, *nz;            /* shading normal = intersect_result::get_normal(), renderer.cpp:430-435 (may be NULL) */
	float *u, *v;                   /* interpolated tex_coord (may be NULL) */
} ptx_hits;
int ptx_intersect_batch(ptx_scene* scene, const ptx_rays* rays, size_t n, const ptx_hits* hits);
/* The same batch with a time per ray (MOTION above: ptx_scene_set_motion): ray i meets every moving model at its transform x(time[i]), on
 * the scene's own route (LDS, hybrid, global, queues), and distance, position and normals of a hit on a moving model are those of that
 * transform. Every output equals, bit for bit, ptx_intersect_batch on the scene set to x(time[i]) with no motion. `time` is host or device
 * memory as the rays are; values are used as given (the states outside [0, 1] are the formula's). On a scene without a moving model `time`
 * is ignored and the call is bitwise ptx_intersect_batch. ptx_intersect_batch itself stays the scene at u = 1: the current transforms. */
int ptx_intersect_batch_motion(ptx_scene* scene, const ptx_rays* rays, const float* time /* [n] */, size_t n, const ptx_hits* hits);

/* Batch form of scene::camera::get_ray(ndc, ratio) (LIB/scene/camera.cpp:10-21): what the integrator kernels compute for every camera
 * sample after the pixel jitter (renderer.cpp:359-370), evaluated by the same device function.
 * in [n][3]: ndc.x, ndc.y, aspect ratio;  out [n][6]: ray origin(3), direction(3). Pointers device or host (both of one kind).
 * It stays the pinhole function of (ndc, ratio) on a scene whose camera has a lens as well. */
int ptx_camera_rays_batch(ptx_scene* scene, const float* ndc_ratio, size_t n, float* rays);
/* The lens branch of THE LENS (ptx_scene_set_camera) with (j.z, j.w) = (u, v), evaluated by the same device function the integrators
 * inline; on a scene without a lens the pinhole rays. in [n][5]: ndc.x, ndc.y, aspect ratio, u, v;  out [n][6]. Pointers and refusals as
 * in ptx_camera_rays_batch. */
int ptx_camera_lens_rays_batch(ptx_scene* scene, const float* in, size_t n, float* rays);
/* The light a punctual candidate at position x with draw u samples, and its pmf_k (PUNCTUAL LIGHTS, PUNCTUAL PICK): the pick alone,
 * evaluated by the same device function the integrators inline, in the scene's mode. In CDF mode the position is ignored: the first
 * entry of the stored CDF with u below it, and the difference of the stored entries. pos_u [n][4]: x(3), u;  light [n], pmf [n]. Pointers
 * device or host, all of one kind. The lights (and the tree) are uploaded if a change is pending. PTX_ERR_NO_DEVICE on a host-only scene;
 * PTX_ERR_INVALID for a NULL scene, NULL pointers with n > 0, mixed kinds and a scene without stored lights. */
int ptx_punctual_pick_batch(ptx_scene* scene, const float* pos_u /* [n][4]: position, u */, size_t n, int32_t* light /* [n] */, float* pmf /* [n] */);
/* The entry of the light list a triangle sample at position x with draw u picks, and its pmf (LIGHT PICK): the stochastic pick alone,
 * evaluated by the same device function the integrator inlines, in the scene's mode. In CDF mode the position is ignored: the first entry
 * of the stored CDF with u below it (clamped to the last), and the difference of the stored entries. pos_u [n][4]: x(3), u; light [n],
 * pmf [n]. Pointer kinds, the upload of pending state and the refusals are those of ptx_punctual_pick_batch: PTX_ERR_NO_DEVICE on a
 * host-only scene; PTX_ERR_INVALID for a NULL scene, NULL pointers with n > 0, mixed pointer kinds and an empty light list. */
int ptx_light_pick_batch(ptx_scene* scene, const float* pos_u /* [n][4]: position, u */, size_t n, int32_t* light /* [n] */, float* pmf /* [n] */);
/* pmf_k(x), the probability with which the pick above returns list entry k = light[i] from position x = pos[i]: the directed evaluation the
 * emission weight inlines. In tree mode it walks the path word of k from the root and multiplies the same branch probabilities in the same
 * order, so it is bit for bit the pmf that ptx_light_pick_batch returns whenever it returns k. In CDF mode the difference of the stored
 * entries. Refusals as above, and PTX_ERR_INVALID for a host `light` entry outside the list (device entries are the caller's to keep
 * inside; an entry outside the list gives pmf 0 and reads nothing). */
int ptx_light_pmf_batch(ptx_scene* scene, const float* pos /* [n][3] */, const int32_t* light /* [n] */, size_t n, float* pmf /* [n] */);

/* Batch form of core::material::get_normal / get_albedo / get_opacity / get_roughness / get_metallic / get_emissive (LIB/core/material.cpp:6-53,
 * bilinear image_texture::sample lookups): what the shading kernels compute at a hit, evaluated by the same device function.
 * surface[n] (surface index in ptx_scene order), uv[n][2];  out[n][12]: normal_ts(3), albedo(3), opacity, roughness, metallic,
 * emissive(3) * 10 (the factor renderer::trace applies, renderer.cpp:462). A surface index outside [0, n_surfaces) gives a row of NaNs.
 * Pointers device or host (all of one kind). */
int ptx_material_eval_batch(ptx_scene* scene, const int32_t* surface, const float* uv, size_t n, float* out);

/* Batch form of the SHADING stage's sampling functions — core::pbr::importance_diffuse / importance_specular / pdf_diffuse /
 * pdf_specular / fresnel (LIB/core/pbr.cpp:71-184), util::rand_cone_vec (LIB/util/rand_cone_vec.cpp:8-35) and core::reflect
 * (LIB/core/utils.hpp:38-40) — evaluated by the same device functions the integrator kernel inlines. Function-level check of the
 * GPU's libm (ocml sin / cos / acos) against the reference's (glibc), and the unit a host SHADING stage queue would call.
 * in [n][14]: normal(3) outcoming(3) incoming(3) u1 u2 roughness cos_theta ior;
 * out[n][15]: rand_cone_vec(u2, cos_theta, normal)(3), importance_diffuse((u1,u2), normal)(3), importance_specular((u1,u2), normal,
 * outcoming, roughness)(3), pdf_diffuse(normal, incoming), pdf_specular(normal, outcoming, incoming, roughness),
 * fresnel(outcoming, reflect(-outcoming, normal), ior), reflect(-outcoming, normal)(3). Pointers device or host (both of one kind). */
int ptx_pbr_eval_batch(ptx_ctx* ctx, const float* in, size_t n, float* out);

/* The leaf loop of core::mesh::intersect (LIB/core/mesh.cpp:381-389: nearest triangle with 0 <= t <= max_dist, the first wins a tie)
 * exactly as the fused kernels run it, on triangles of the caller's choosing: the records are built by the scene builder's own code
 * and the kernel calls the traversal on a tree of one leaf holding all n_tri triangles (1 <= n_tri <= 256), so the short reciprocal,
 * its range bookkeeping and the IEEE re-test of the whole leaf are the shipped ones.
 * corners[n_tri][9]: a, b, c;  refs[n_tri]: the leaf's reference list, a permutation of 0 .. n_tri-1 (NULL: the identity);
 * leaf_ordered = 0: one record per triangle behind the references (the ref-indexed LDS-resident layout), 2: one record per reference,
 * in leaf order, staged into LDS without references (the leaf-ordered LDS-resident layout), any other value: one record per reference, in
 * leaf order, carrying its triangle id (the global-memory layout);  rays[n_rays][7]: origin, unit direction, max_dist.
 * out[n_rays][3]: t, beta, gamma (-1, 0, 0 on a miss);  triangle[n_rays]: index into corners, -1 on a miss. Host memory only. */
int ptx_leaf_intersect_batch(ptx_ctx* ctx, const float* corners, uint32_t n_tri, const uint32_t* refs, int leaf_ordered, const float* rays, size_t n_rays,
                             float* out, int32_t* triangle);

/* Self-check of the short reciprocal / square-root sequences the kernels use in place of the IEEE ones (device_core.hpp), as compiled
 * into this library, guards and fallbacks included: every float pattern through each form. mismatches[3] receives, per form, the
 * count of results whose bits differ from the IEEE expression (NaN equals NaN): 1.0f / x, sqrtf(x), 1.0f / sqrtf(x). All zero when
 * the sequences are exact. */
int ptx_exact_math_check(ptx_ctx* ctx, uint64_t* mismatches);

/* Self-check of the per-material constants of the shade records: the scene builder computes, once per surface, what a path vertex
 * needs of the material's roughness and ior alone (roughness^4 of the clamped roughness, that minus 1, the Smith k, the squared
 * Fresnel f0), and the untextured kernels read them instead of computing them. materials[n][9]: roughness, metallic, ior, albedo rgb,
 * emissive rgb (the record holds nothing of the last seven; they are ignored). For every row the builder's own function fills a record
 * on the host and the device evaluates the vertex's expressions; *mismatches receives the number of words whose bits differ (NaN
 * equals NaN). Zero when the records hold what the vertex would compute. Host memory only. */
int ptx_shade_consts_check(ptx_ctx* ctx, const float* materials, size_t n, uint64_t* mismatches);

/* ---- multi-GPU fan-in ------------------------------------------------------------------------------
 * The one exchange step of the path: the sum of the per-rank accumulation buffers on rank `root`. Replaces the
 * reference's planned (never implemented) SNS/SQS result fan-in (src/models/work_info.hpp:22-23,
 * src/processors/worker/intersection_worker.cpp:69-147). `nccl_comm` is an RCCL communicator the host created
 * (ncclCommInitRank: one rank per GPU); the library does not link RCCL, it resolves ncclReduce from the RCCL the
 * process has already loaded (or from librccl.so) at the first call, and enqueues
 * ncclReduce(accum, accum, n_floats, ncclFloat32, ncclSum, root, comm, ptx_ctx_stream(ctx)) — in place, device memory.
 * Call ptx_ctx_synchronize (or chain work on that stream) before reading the result. PTX_ERR_UNSUPPORTED when no RCCL
 * can be found, PTX_ERR_HIP when RCCL reports an error. */
int ptx_reduce_framebuffer(ptx_ctx* ctx, void* nccl_comm, float* accum_rgba, size_t n_floats, int root);

/* ---- image write --------------------------------------------------------------------------------
 * Replaces the tonemap + image::write loop of renderer.cpp:409-424 (core::tonemap_approx_aces,
 * LIB/core/utils.hpp:29-36; image::image::write, LIB/image/image.cpp:143-154): divides the sums by
 * `spp`, applies ACES, sRGB (pow 1/2.2) and quantises to RGBA8 row-major; alpha is quantised linearly. accum/rgba8 device or host.
 * With spp = 1 it writes the means of ptx_render_transparent unchanged (x / 1.0f is exact). */
int ptx_tonemap_encode(ptx_ctx* ctx, const float* accum_rgba, uint32_t W, uint32_t H, uint32_t spp, uint8_t* rgba8);
/* Replaces image::image::save_to_memory_png (LIB/image/image.cpp:111-122). Host memory only.
 * *png is malloc'ed; release with ptx_free. Decoded pixels are exact; the byte stream is zlib's, not stb's. */
int ptx_encode_png(const uint8_t* rgba8, uint32_t W, uint32_t H, uint8_t** png, size_t* png_bytes);
void ptx_free(void* p);

/* ---- multi-GPU ----------------------------------------------------------------------------------
 * The reference's planned fan-in (SNS/SQS, never implemented: src/models/work_info.hpp:22-23) is replaced
 * by ONE sum-reduce of the float accumulation buffer. The library does not own a communicator:
 * torch.distributed (backend "nccl" = RCCL over xGMI) reduces the device buffer ptx_render filled; see
 * INTEGRATION.md. */

#ifdef __cplusplus
}
#endif
#endif /* PTX_H */
