"""Seeded procedural scenes (numpy only) for the BASELINE configs whose assets the reference does not ship
(no Stanford bunny anywhere, `sponza.bin` missing): displaced icospheres of a chosen triangle
count, placed either in the reference's Cornell room or on an open sun-lit plaza. Every generator is
deterministic, so the GPU box regenerates identical geometry. Output = the flat arrays both
`Scene.from_arrays` (product) and the oracle's `SceneArrays` take."""
import numpy as np

_T = (1.0 + 5.0 ** 0.5) / 2.0


def icosphere(level: int):
    """Unit icosphere: 20 * 4**level triangles (level 6 -> 81 920, level 7 -> 327 680)."""
    v = np.array([[-1, _T, 0], [1, _T, 0], [-1, -_T, 0], [1, -_T, 0], [0, -1, _T], [0, 1, _T], [0, -1, -_T], [0, 1, -_T],
                  [_T, 0, -1], [_T, 0, 1], [-_T, 0, -1], [-_T, 0, 1]], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int64)
    for _ in range(level):
        n = len(v)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = np.sort(e, axis=1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        v = np.concatenate([v, mid])
        m = (n + inv.reshape(3, -1).T)            # midpoint ids per face: ab, bc, ca
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ab, bc, ca = m[:, 0], m[:, 1], m[:, 2]
        f = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
    return v, f


def displaced_icosphere(level: int, seed: int = 1, amplitude: float = 0.15):
    """-> vertices [n,11] float32 (position, uv, normal, tangent), triangles [m,3] uint32.
    Displacement: a few seeded low-frequency lobes along the normal (keeps the mesh a star-shaped solid)."""
    v, f = icosphere(level)
    rng = np.random.default_rng(seed)
    r = np.ones(len(v))
    for _ in range(6):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        k = rng.integers(2, 7)
        r += amplitude / 6 * np.cos(k * np.arccos(np.clip(v @ d, -1, 1)) + rng.uniform(0, 6.28))
    p = v * r[:, None]
    # area-weighted vertex normals
    fn = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    nrm = np.zeros_like(p)
    for k in range(3):
        np.add.at(nrm, f[:, k], fn)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
    up = np.where(np.abs(nrm[:, 1:2]) < 0.99, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    tan = np.cross(up, nrm)
    tan /= np.maximum(np.linalg.norm(tan, axis=1, keepdims=True), 1e-20)
    uv = np.stack([np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5, np.arcsin(np.clip(v[:, 1], -1, 1)) / np.pi + 0.5], 1)
    out = np.concatenate([p, uv, nrm, tan], 1).astype(np.float32)
    return out, f.astype(np.uint32)


def _quad(y, half, normal_up=True):
    p = np.array([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]], np.float32)
    n = np.array([0, 1, 0], np.float32)
    v = np.zeros((4, 11), np.float32)
    v[:, 0:3] = p
    v[:, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
    v[:, 5:8] = n
    v[:, 8:11] = [1, 0, 0]
    t = np.array([[0, 2, 1], [0, 3, 2]], np.uint32)   # counter-clockwise seen from +y
    return v, t


def _look_at(eye, target):
    """Camera basis columns (x, y, z) with -z pointing at the target, as scene::camera expects (camera.cpp:10-21)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0, 1, 0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([eye, x, y, z]).astype(np.float32)


def plaza_scene(level: int = 3, sun: bool = True, alpha: bool = True, seed: int = 3):
    """Open scene: ground quad (shadow catcher when `alpha`), a displaced icosphere (scaled + translated model, glossy
    metal), a second small sphere (half-transparent when `alpha`), one directional light when `sun`.
    -> dict of arrays: model_xform, model_surf, surf_range, vertices, triangles, materials, camera[13], sun[13] or None."""
    gv, gt = _quad(0.0, 6.0)
    s1v, s1t = displaced_icosphere(level, seed, 0.2)
    s2v, s2t = displaced_icosphere(max(level - 1, 0), seed + 1, 0.05)
    verts = np.concatenate([gv, s1v, s2v])
    tris = np.concatenate([gt, s1t, s2t])
    surf_range = np.array([[0, len(gv), 0, len(gt)], [len(gv), len(s1v), len(gt), len(s1t)],
                           [len(gv) + len(s1v), len(s2v), len(gt) + len(s1t), len(s2t)]], np.int32)
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    model_xform = np.array([[0, 0, 0] + ident,
                            [0.3, 1.25, -0.2, 1.1, 0, 0, 0, 1.1, 0, 0, 0, 1.1],
                            [-1.9, 0.62, 1.1, 0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6]], np.float32)
    model_surf = np.array([[0, 1], [1, 1], [2, 1]], np.int32)
    #            albedo            opacity rough metal emissive     ior   shadow_catcher
    materials = np.array([[0.75, 0.72, 0.68, 1.0, 0.6, 0.0, 0, 0, 0, 1.33, 1.0 if alpha else 0.0],
                          [0.95, 0.64, 0.54, 1.0, 0.25, 1.0, 0, 0, 0, 1.33, 0.0],
                          [0.2, 0.5, 0.9, 0.55 if alpha else 1.0, 0.4, 0.0, 0.05, 0.05, 0.1, 1.33, 0.0]], np.float32)
    cam = np.concatenate([_look_at([4.5, 3.2, 6.5], [0.0, 0.9, 0.0]), [np.float32(0.7)]]).astype(np.float32)
    sun13 = None
    if sun:
        d = np.array([0.35, 0.8, 0.45])   # direction TOWARDS the sun = basis * (0,0,1) (renderer.cpp:499)
        d /= np.linalg.norm(d)
        x = np.cross([0, 1, 0], d)
        x /= np.linalg.norm(x)
        y = np.cross(d, x)
        sun13 = np.concatenate([x, y, d, [3.0, 2.7, 2.2], [0.004732]]).astype(np.float32)
    return dict(model_xform=model_xform, model_surf=model_surf, surf_range=surf_range, vertices=verts.astype(np.float32),
                triangles=tris.astype(np.uint32), materials=materials, camera=cam, sun=sun13)


def cornell_with_mesh(cornell: dict, level: int = 6, seed: int = 7):
    """The reference's Cornell room (arrays as loaded from scenes/cornell-box) with its 960-triangle sphere replaced by
    a displaced icosphere of 20*4**level triangles: the "~70k-triangle mesh, KD-tree traversal stress" of BASELINE
    config 3 (level 6 = 81 920 triangles) and, at level 7 (327 680), the "~250k-triangle" class of configs 4-5."""
    sr = np.asarray(cornell["surf_range"])[:, :4]
    keep = len(sr) - 1                                  # the sphere is the last surface / model
    v0, nv, t0, nt = sr[keep]
    mv, mt = displaced_icosphere(level, seed, 0.12)
    verts = np.concatenate([np.asarray(cornell["vertices"])[:v0], mv])
    tris = np.concatenate([np.asarray(cornell["triangles"])[:t0], mt])
    surf_range = np.concatenate([sr[:keep], [[v0, len(mv), t0, len(mt)]]]).astype(np.int32)
    return dict(model_xform=np.asarray(cornell["model_xform"], np.float32), model_surf=np.asarray(cornell["model_surf"], np.int32),
                surf_range=surf_range, vertices=verts.astype(np.float32), triangles=tris.astype(np.uint32),
                materials=np.asarray(cornell["materials"], np.float32), camera=np.asarray(cornell["camera"], np.float32)[:13], sun=None)


def _grid(n: int, origin, du, dv):
    """n x n quads (2 n^2 triangles) spanning origin + s*du + t*dv, s,t in [0,1]; normal = normalize(du x dv)."""
    origin, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    s, t = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing="ij")
    p = origin + s[..., None] * du + t[..., None] * dv
    nrm = np.cross(du, dv)
    nrm /= np.linalg.norm(nrm)
    tan = du / np.linalg.norm(du)
    v = np.zeros(((n + 1) ** 2, 11), np.float32)
    v[:, 0:3] = p.reshape(-1, 3)
    v[:, 3:5] = np.stack([s, t], -1).reshape(-1, 2)
    v[:, 5:8] = nrm
    v[:, 8:11] = tan
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    b, c, d = a + (n + 1), a + (n + 1) + 1, a + 1
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.uint32)
    return v, tri


def _place(v, scale, offset):
    """Scale + translate a vertex array in place of a node transform (one model, many surfaces); normals by the inverse-transpose."""
    out = v.copy()
    sc = np.asarray(scale, np.float32)
    out[:, 0:3] = v[:, 0:3] * sc + np.asarray(offset, np.float32)
    n = v[:, 5:8] / sc
    out[:, 5:8] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    t = v[:, 8:11] * sc
    out[:, 8:11] = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-20)
    return out


def atrium_scene(detail: int = 5, seed: int = 11):
    """Sponza-class stand-in for BASELINE configs 4-5 (`sponza.bin` is missing from the reference): ONE model with 24 surfaces
    (as Sponza's single mesh has 24 primitives) — a gridded floor and three walls, two rows of five tall columns, eight
    ornaments, a lintel and a plinth — lit by one directional light through the open roof. detail = 5 gives 262 176 triangles
    (Sponza's accessors total 262 267); every level down divides the sphere-derived part by four."""
    parts = []
    g = max(detail - 1, 0)
    parts.append(_grid(4 << g, [-6, 0, -14], [0, 0, 28], [12, 0, 0]))                 # floor, normal +y
    parts.append(_grid(2 << g, [-6, 0, -14], [0, 9, 0], [0, 0, 28]))                  # left wall, normal +x
    parts.append(_grid(2 << g, [6, 0, 14], [0, 9, 0], [0, 0, -28]))                   # right wall, normal -x
    parts.append(_grid(2 << g, [-6, 0, -14], [12, 0, 0], [0, 9, 0]))                  # back wall, normal +z
    col_v, col_t = displaced_icosphere(detail, seed, 0.10)
    for k in range(10):
        x = -3.2 if k % 2 == 0 else 3.2
        z = -11.0 + 5.0 * (k // 2)
        parts.append((_place(col_v, (0.55, 3.6, 0.55), (x, 3.6, z)), col_t))
    orn_v, orn_t = displaced_icosphere(max(detail - 1, 0), seed + 1, 0.25)
    for k in range(8):
        x = -1.6 + 3.2 * (k % 2)
        z = -9.0 + 5.5 * (k // 2)
        parts.append((_place(orn_v, (0.7, 0.7, 0.7), (x, 0.75 + 0.5 * (k % 3), z)), orn_t))
    parts.append(_grid(1 << g, [-6, 8.2, -14], [12, 0, 0], [0, 0, 6]))                # lintel over the far end, normal -y
    parts.append(_grid((7 << g) // 4 or 1, [-2, 0.02, 6], [0, 0, 4], [4, 0, 0]))      # plinth, normal +y
    assert len(parts) == 24
    verts = np.concatenate([p[0] for p in parts]).astype(np.float32)
    tris = np.concatenate([p[1] for p in parts]).astype(np.uint32)
    sr, v0, t0 = [], 0, 0
    for v, t in parts:
        sr.append([v0, len(v), t0, len(t)])
        v0 += len(v); t0 += len(t)
    rng = np.random.default_rng(seed)
    mats = np.zeros((24, 11), np.float32)
    mats[:, 0:3] = 0.35 + 0.55 * rng.random((24, 3))
    mats[:, 3] = 1.0
    mats[:, 4] = 0.25 + 0.7 * rng.random(24)
    mats[4:14, 5] = (rng.random(10) < 0.3)            # a few metallic columns
    mats[:, 9] = 1.45
    d = np.array([0.25, 0.85, 0.35])                  # towards the sun
    d /= np.linalg.norm(d)
    x = np.cross([0, 1, 0], d); x /= np.linalg.norm(x)
    y = np.cross(d, x)
    sun13 = np.concatenate([x, y, d, [4.0, 3.7, 3.2], [0.004732]]).astype(np.float32)
    cam = np.concatenate([_look_at([0.3, 2.2, 13.0], [0.0, 2.6, -6.0]), [np.float32(0.9)]]).astype(np.float32)
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    return dict(model_xform=np.array([[0, 0, 0] + ident], np.float32), model_surf=np.array([[0, 24]], np.int32),
                surf_range=np.array(sr, np.int32), vertices=verts, triangles=tris, materials=mats, camera=cam, sun=sun13)


def _rotation(rng):
    """Uniformly random rotation matrix (QR of a Gaussian matrix, signs fixed so that det = +1)."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _corners(half):
    return np.array([[sx, sy, sz] for sx in (-half, half) for sy in (-half, half) for sz in (-half, half)], np.float64)


def cloud_scene(n_models: int = 1, surfaces_per_model: int = 64, tris_per_surface: int = 16, seed: int = 5,
                layout: str = "overlap", spaces=None, tri_size: float = 0.08):
    """Many surfaces of small random triangles, for the per-surface / per-model limits of the kernels (surface masks and
    deferral lists are 64 lanes or bits wide). n_models models of surfaces_per_model surfaces each (surface u = m *
    surfaces_per_model + k), tris_per_surface triangles per surface, one directional light.
    Every model has its own transform (rotation, non-uniform scale, translation); with `spaces` = k, model m takes transform
    m % k (A, B, A, B, ...: several models share a ray space, not next to each other). The geometry is laid out in WORLD space
    and stored in the model's local space (inverse transform), so the layout does not depend on the transforms:
      "overlap":   every surface spreads its triangles over the same cube [-1, 1]^3, with a vertex on each of the cube's corners
                   (the convex hull of every surface's vertices is the whole cube, so every surface box, in any ray space, contains
                   every point of it). The camera sits near the centre: every camera ray enters every surface box.
      "scattered": each surface is a small cluster on a grid in front of the camera: a ray enters a few boxes at most.
    At 16 triangles per surface, 64-65 surfaces fit one CU's LDS (the fused kernel's LDS route); at 24 the scene is hybrid.
    -> dict of arrays as plaza_scene (vertices [n, 11]: position, uv, normal, tangent)."""
    if layout not in ("overlap", "scattered"):
        raise ValueError(f"layout must be 'overlap' or 'scattered', not {layout!r}")
    n_surf = n_models * surfaces_per_model
    if layout == "overlap" and tris_per_surface < 8:
        raise ValueError("'overlap' needs at least 8 triangles per surface (one at each corner of the cube)")
    rng = np.random.default_rng(seed)
    n_xf = n_models if spaces is None else int(spaces)
    xforms = []
    for _ in range(n_xf):
        rot = _rotation(rng)
        scale = rng.uniform(0.6, 1.6, 3)
        basis = rot * scale[None, :]                      # world = basis @ local + origin
        origin = rng.uniform(-0.5, 0.5, 3)
        xforms.append((basis.astype(np.float32).astype(np.float64), origin.astype(np.float32).astype(np.float64)))
    if layout == "scattered":
        cols = int(np.ceil(np.sqrt(n_surf)))
        rows = (n_surf + cols - 1) // cols
    verts, tris, sr = [], [], []
    v0 = t0 = 0
    for m in range(n_models):
        basis, origin = xforms[m % n_xf]
        inv = np.linalg.inv(basis)
        for k in range(surfaces_per_model):
            u = m * surfaces_per_model + k
            if layout == "overlap":
                centres = rng.uniform(-0.95, 0.95, (tris_per_surface, 3))
                centres[:8] = _corners(0.95)
                size = tri_size
            else:
                r, c = divmod(u, cols)
                cell = np.array([(c - (cols - 1) / 2) * 0.5, (r - (rows - 1) / 2) * 0.5, rng.uniform(-0.2, 0.2)])
                centres = cell + rng.uniform(-0.12, 0.12, (tris_per_surface, 3))
                size = tri_size
            p = centres[:, None, :] + rng.uniform(-size, size, (tris_per_surface, 3, 3))
            if layout == "overlap":                       # corner triangles: one vertex ON the corner, two inside the cube
                c8 = _corners(1.0)
                p[:8] = c8[:, None, :] - np.sign(c8)[:, None, :] * rng.uniform(0.0, 2.0 * size, (8, 3, 3))
                p[:8, 0] = c8
            p = p.reshape(-1, 3)
            fn = np.cross(p[1::3] - p[0::3], p[2::3] - p[0::3])
            fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
            tw = p[1::3] - p[0::3]
            tw /= np.maximum(np.linalg.norm(tw, axis=1, keepdims=True), 1e-20)
            v = np.zeros((3 * tris_per_surface, 11), np.float64)
            v[:, 0:3] = (p - origin) @ inv.T                 # local = inv(basis) (world - origin)
            v[:, 3:5] = rng.random((3 * tris_per_surface, 2))
            nl = np.repeat(fn, 3, axis=0) @ basis            # normals by the transpose: inv(basis)^T (basis^T n) = n
            v[:, 5:8] = nl / np.linalg.norm(nl, axis=1, keepdims=True)
            tl = np.repeat(tw, 3, axis=0) @ inv.T            # tangents as positions
            v[:, 8:11] = tl / np.linalg.norm(tl, axis=1, keepdims=True)
            verts.append(v)
            tris.append(np.arange(3 * tris_per_surface).reshape(-1, 3))
            sr.append([v0, len(v), t0, tris_per_surface])
            v0 += len(v)
            t0 += tris_per_surface
    model_xform = np.array([np.concatenate([xforms[m % n_xf][1], xforms[m % n_xf][0].T.ravel()]) for m in range(n_models)], np.float32)
    model_surf = np.array([[m * surfaces_per_model, surfaces_per_model] for m in range(n_models)], np.int32)
    mats = np.zeros((n_surf, 11), np.float32)
    mats[:, 0:3] = 0.3 + 0.6 * rng.random((n_surf, 3))
    mats[:, 3] = 1.0
    mats[:, 4] = 0.2 + 0.7 * rng.random(n_surf)
    mats[:, 5] = rng.random(n_surf) < 0.25
    mats[:, 9] = 1.45
    d = np.array([0.3, 0.8, 0.5])                    # towards the sun
    d /= np.linalg.norm(d)
    x = np.cross([0, 1, 0], d); x /= np.linalg.norm(x)
    y = np.cross(d, x)
    sun13 = np.concatenate([x, y, d, [3.0, 2.8, 2.5], [0.004732]]).astype(np.float32)
    if layout == "overlap":
        cam = _look_at([0.02, 0.01, 0.03], [0.3, -0.1, -1.0])
    else:
        cam = _look_at([0.1, 0.05, 4.5], [0.0, 0.0, 0.0])
    cam = np.concatenate([cam, [np.float32(1.0 if layout == "overlap" else 0.8)]]).astype(np.float32)
    return dict(model_xform=model_xform, model_surf=model_surf, surf_range=np.array(sr, np.int32),
                vertices=np.concatenate(verts).astype(np.float32), triangles=np.concatenate(tris).astype(np.uint32),
                materials=mats, camera=cam, sun=sun13)


def emitter_cloud_scene(sun: bool = True, alpha: bool = True, seed: int = 17):
    """cloud_scene(3, 21, 16, layout="scattered", tri_size=0.15) with many small emitters, for ptx_render_nee's light list: a list of a
    few hundred triangles spread over surfaces far from index 0, under three rotated, non-uniformly scaled models.
      emissive:  surfaces u % 4 == 1, surface 0 and surface 62, factors in [0.05, 0.45]; surface 5 has one non-zero channel only.
      surface 9: opacity 0.5 when `alpha` (an emitter that must stay off the list: the only pass-through material), opaque otherwise.
      triangle 5 of surface 1 is collapsed to zero area (its third corner moved onto its second): the list has a gap there.
      a fourth model of one surface, under a transform of its own: a 6 x 6 receiver quad at world z = -0.6 behind the cloud, facing
      the camera. 64 surfaces in all, so the queue route still takes the scene.
      sun:       False removes the directional light.
    -> dict of arrays as cloud_scene, plus `emissive` (surface ids), `unlisted` (emissive surfaces that must not be listed) and
    `collapsed` ((surface, triangle))."""
    d = cloud_scene(3, 21, 16, layout="scattered", tri_size=0.15)
    rng = np.random.default_rng(seed)
    mats = d["materials"].copy()
    n_cloud = len(mats)
    emissive = sorted({u for u in range(n_cloud) if u % 4 == 1} | {0, n_cloud - 1})
    mats[emissive, 6:9] = rng.uniform(0.05, 0.45, (len(emissive), 3)).astype(np.float32)
    mats[5, 6], mats[5, 8] = 0.0, 0.0
    if alpha:
        mats[9, 3] = 0.5
    verts = d["vertices"].copy()
    v0, _, t0, _ = (int(x) for x in d["surf_range"][1][:4])
    c = v0 + d["triangles"][t0 + 5].astype(np.int64)
    verts[c[2], 0:3] = verts[c[1], 0:3]
    # the receiver: laid out in world space, stored in its model's local space, as cloud_scene does
    basis = (_rotation(rng) * rng.uniform(0.6, 1.6, 3)[None, :]).astype(np.float32).astype(np.float64)
    origin = rng.uniform(-0.5, 0.5, 3).astype(np.float32).astype(np.float64)
    inv = np.linalg.inv(basis)
    p = np.array([[-3, -3, -0.6], [3, -3, -0.6], [3, 3, -0.6], [-3, 3, -0.6]], np.float64)
    q = np.zeros((4, 11), np.float64)
    q[:, 0:3] = (p - origin) @ inv.T
    q[:, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
    nl = np.array([0.0, 0.0, 1.0]) @ basis
    q[:, 5:8] = nl / np.linalg.norm(nl)
    tl = np.array([1.0, 0.0, 0.0]) @ inv.T
    q[:, 8:11] = tl / np.linalg.norm(tl)
    nv, nt = len(verts), len(d["triangles"])
    quad_mat = np.array([[0.7, 0.7, 0.65, 1.0, 0.6, 0.0, 0, 0, 0, 1.45, 0]], np.float32)
    return dict(model_xform=np.concatenate([d["model_xform"], np.concatenate([origin, basis.T.ravel()])[None].astype(np.float32)]),
                model_surf=np.concatenate([d["model_surf"], np.array([[n_cloud, 1]], np.int32)]),
                surf_range=np.concatenate([d["surf_range"], np.array([[nv, 4, nt, 2]], np.int32)]),
                vertices=np.concatenate([verts, q.astype(np.float32)]),
                triangles=np.concatenate([d["triangles"], np.array([[0, 1, 2], [0, 2, 3]], np.uint32)]),
                materials=np.concatenate([mats, quad_mat]), camera=d["camera"], sun=d["sun"] if sun else None,
                emissive=np.array(emissive, np.int32), unlisted=np.array([9] if alpha else [], np.int32), collapsed=(1, 5))


# ---------------------------------------------------------------------------- the material chart
_NEAR1 =float(np.nextafter(np.float32(1), np.float32(0)))
_BASE = (0.9, 0.6, 0.3)
# One patch per regime of the shading vertex: (name, albedo, opacity, roughness, metallic, emissive, ior, shadow catcher, flipped).
# The three opacities next to 1 all fall on the `is_approx(opacity, 1)` side of renderer.cpp:466 (|opacity - 1| < 0.0001): opaque.
CHART_REGIMES = (
    [(f"rough{r:g}_metal{m:g}", _BASE, 1.0, r, m, (0, 0, 0), 1.33, 0, False) for r in (0.0, 0.01, 0.05, 0.3, 1.0) for m in (0.0, 0.5, 1.0)]
    + [(f"opacity_{tag}", (0.3, 0.7, 0.9), op, 0.5, 0.0, em, 1.33, 0, False)      # emissive and half-transparent: the worker adds it first
       for tag, op, em in (("0", 0.0, (0, 0, 0)), ("0.5", 0.5, (0.05, 0.02, 0.01)), ("below1", _NEAR1, (0, 0, 0)),
                           ("1m5e-7", 1 - 5e-7, (0, 0, 0)), ("1m2e-6", 1 - 2e-6, (0, 0, 0)))]
    + [("emissive_dielectric", (0.6, 0.6, 0.6), 1.0, 0.5, 0.0, (0.5, 0.3, 0.1), 1.33, 0, False),
       ("emissive_metal", (0.9, 0.7, 0.4), 1.0, 0.3, 1.0, (0.2, 0.4, 0.8), 1.33, 0, False),
       ("albedo0", (0.0, 0.0, 0.0), 1.0, 0.5, 0.0, (0, 0, 0), 1.33, 0, False),
       ("albedo1", (1.0, 1.0, 1.0), 1.0, 0.5, 0.0, (0, 0, 0), 1.33, 0, False),
       ("ior1", _BASE, 1.0, 0.3, 0.0, (0, 0, 0), 1.0, 0, False),
       ("ior2.5", _BASE, 1.0, 0.3, 0.0, (0, 0, 0), 2.5, 0, False),
       ("backface", _BASE, 1.0, 0.5, 0.0, (0.1, 0.1, 0.1), 1.33, 0, True),
       ("catcher", (0.7, 0.7, 0.7), 1.0, 0.6, 0.0, (0, 0, 0), 1.33, 1, False),            # columns 3 and 4: in the blocker's shadow
       ("catcher_opacity0.5", (0.7, 0.7, 0.7), 0.5, 0.6, 0.0, (0, 0, 0), 1.33, 1, False)]
)
CHART_COLS, CHART_ROWS, CHART_HALF = 6, 5, 0.45       # unit cells centred on the origin, patches of 0.9 x 0.9: gaps of 0.1
CHART_EYE, CHART_FOV = (0.0137, 1.6, -0.0091), 2.0    # the 5 cells of a column fill the frame's height; off the cell grid
CHART_TOP = 6.4                                       # height of the facing chart (the camera is below it)
CHART_SUN_DIR = (0.5, 0.866, 0.05)
CHART_BLOCKER = (1.3, 1.3 * 0.5 / 0.866, 5.1, -3.4, 3.4)   # y, x0, x1, z0, z1: the shadow of the edge x0 falls on x = 0


def chart_scene(sun=None, blocker=False, facing=False, alpha=True):
    """Material chart: one square patch (two triangles, its own surface and material) per row of CHART_REGIMES, coplanar on y = 0 with
    normals up, in open space, seen straight down by a camera at CHART_EYE (row `backface` has winding and normals turned over).
    Patch k sits in cell (k % 6, k // 6) of the full table whatever the options, one model for everything.
      sun:     None, or the angular radius of one directional light (towards CHART_SUN_DIR, 60 degrees above the plane).
      blocker: one opaque quad at y = 1.3 over x >= 0.75, outside the camera's view of every patch. With a sharp sun its shadow ends at
               x = 0, in the gap between columns 2 and 3: columns 3-5 are shadowed, columns 0-2 lit. A sun of radius 0.5 leaves columns
               4-5 wholly in the umbra (the quad reaches 2.1 past them in x and 0.95 in z) and column 0 wholly lit.
      facing:  a second chart at y = CHART_TOP, above the camera, normals down, same materials: bounce rays hit it or leave through
               the gaps (and it shadows parts of the lower chart from the sun).
      alpha:   False leaves out every patch with an opacity below 1 or a shadow catcher (no material can pass a ray through).
    -> dict of arrays as plaza_scene, plus `names` (per surface) and `cells` (per surface: column, row, level; -1 for the blocker)."""
    rows = [r for r in CHART_REGIMES if alpha or (r[2] == 1.0 and not r[7])]
    cell = {r[0]: divmod(k, CHART_COLS)[::-1] for k, r in enumerate(CHART_REGIMES)}
    verts, tris, mats, names, cells = [], [], [], [], []

    def add(name, x0, x1, z0, z1, y, up, mat, where):
        v = np.zeros((4, 11), np.float32)
        v[:, 0:3] = [[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]]
        v[:, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
        v[:, 5:8] = [0, 1 if up else -1, 0]
        v[:, 8:11] = [1, 0, 0]
        verts.append(v)
        tris.append(np.array([[0, 2, 1], [0, 3, 2]] if up else [[0, 1, 2], [0, 2, 3]], np.uint32))   # counter-clockwise seen from the normal's side
        mats.append(mat); names.append(name); cells.append(where)
    for level in range(2 if facing else 1):
        for name, alb, op, rough, metal, em, ior, catcher, flipped in rows:
            cx, cz = cell[name][0] - (CHART_COLS - 1) / 2, cell[name][1] - (CHART_ROWS - 1) / 2
            add(name + ("_top" if level else ""), cx - CHART_HALF, cx + CHART_HALF, cz - CHART_HALF, cz + CHART_HALF, CHART_TOP * level,
                (level == 0) != flipped, [*alb, op, rough, metal, *em, ior, catcher], (*cell[name], level))
    if blocker:
        y, x0, x1, z0, z1 = CHART_BLOCKER
        add("blocker", x0, x1, z0, z1, y, True, [0.5, 0.5, 0.5, 1.0, 0.5, 0.0, 0, 0, 0, 1.33, 0], (-1, -1, -1))
    n = len(verts)
    sun13 = None
    if sun is not None:
        d = np.array(CHART_SUN_DIR) / np.linalg.norm(CHART_SUN_DIR)
        x = np.cross([0, 1, 0], d); x /= np.linalg.norm(x)
        sun13 = np.concatenate([x, np.cross(d, x), d, [3.0, 2.7, 2.2], [sun]]).astype(np.float32)
    cam = np.array([*CHART_EYE, 1, 0, 0, 0, 0, -1, 0, 1, 0, CHART_FOV], np.float32)      # -z of the camera points down, image up is world -z
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    return dict(model_xform=np.array([[0, 0, 0] + ident], np.float32), model_surf=np.array([[0, n]], np.int32),
                surf_range=np.array([[4 * k, 4, 2 * k, 2] for k in range(n)], np.int32), vertices=np.concatenate(verts),
                triangles=np.concatenate(tris), materials=np.array(mats, np.float32), camera=cam, sun=sun13,
                names=names, cells=np.array(cells, np.int32))


# ---------------------------------------------------------------------------- lamps (punctual lights, ptx_scene_set_punctual_lights)
LAMP_BLOCKER = (1.0, 0.3, 1.5, -0.9, 0.9)   # y, x0, x1, z0, z1 of the floor scene's blocker quad
LAMP_FIRST = (-0.6, 2.0, 0.3)               # lamp 0 of every lamp_scene: left of the blocker, whose shadow then falls on x > 0.7 of the floor


def lamp_scene(n_lamps: int = 1, chart: bool = False, emitters: bool = False, blocker: bool = True, spots: bool = False, lamp_range: float = 0.0,
               power: float = 10.0, seed: int = 23):
    """A scene lit by point and spot lights -> (dict of arrays as plaza_scene, lights [n_lamps, 16] float32 for Scene.set_punctual_lights).
      chart:    False: a diffuse floor (8 x 8 on y = 0) seen from above at an angle, a blocker quad at y = 1 (LAMP_BLOCKER) when `blocker`, and
                with `emitters` one small bright emissive quad (0.2 x 0.2) at y = 3 facing down. True: chart_scene(facing=True, alpha=False), its emissive
                factors set to zero unless `emitters`.
      lamps:    lamp 0 at LAMP_FIRST, the others scattered (seeded) over |x|, |z| < 2.2 at heights 1.4 .. 2.6 (chart: 2 .. 4.4, between
                the two charts); colours in [0.4, 1], intensities log-uniform over a decade around power / n_lamps.
      spots:    odd lamps (all of them when n_lamps == 1) are spots shining down, tilted by up to 0.35 rad, cones 0.35 / 0.6 rad.
      lamp_range: the range field of every lamp (0 = unlimited)."""
    rng = np.random.default_rng(seed)
    if chart:
        d = chart_scene(facing=True, alpha=False, blocker=blocker)
        if not emitters:
            d["materials"] = d["materials"].copy()
            d["materials"][:, 6:9] = 0
        y_lo, y_hi = 2.0, 4.4
    else:
        verts, tris, mats = [], [], []

        def add(x0, x1, z0, z1, y, up, mat):
            v = np.zeros((4, 11), np.float32)
            v[:, 0:3] = [[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]]
            v[:, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
            v[:, 5:8] = [0, 1 if up else -1, 0]
            v[:, 8:11] = [1, 0, 0]
            verts.append(v)
            tris.append(np.array([[0, 2, 1], [0, 3, 2]] if up else [[0, 1, 2], [0, 2, 3]], np.uint32))
            mats.append(mat)
        add(-4, 4, -4, 4, 0.0, True, [0.7, 0.7, 0.7, 1.0, 0.6, 0.0, 0, 0, 0, 1.33, 0])
        if blocker:
            y, x0, x1, z0, z1 = LAMP_BLOCKER
            add(x0, x1, z0, z1, y, True, [0.4, 0.5, 0.6, 1.0, 0.5, 0.0, 0, 0, 0, 1.33, 0])
        if emitters:
            add(-1.7, -1.5, -1.4, -1.2, 3.0, False, [0.8, 0.8, 0.8, 1.0, 0.5, 0.0, 5.0, 4.5, 3.5, 1.33, 0])
        n = len(verts)
        ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        cam = np.concatenate([_look_at([0.0, 5.0, 4.5], [0.0, 0.0, 0.0]), [np.float32(0.8)]]).astype(np.float32)
        d = dict(model_xform=np.array([[0, 0, 0] + ident], np.float32), model_surf=np.array([[0, n]], np.int32),
                 surf_range=np.array([[4 * k, 4, 2 * k, 2] for k in range(n)], np.int32), vertices=np.concatenate(verts),
                 triangles=np.concatenate(tris), materials=np.array(mats, np.float32), camera=cam, sun=None)
        y_lo, y_hi = 1.4, 2.6
    lights = np.zeros((n_lamps, 16), np.float32)
    for k in range(n_lamps):
        pos = LAMP_FIRST if k == 0 else (rng.uniform(-2.2, 2.2), rng.uniform(y_lo, y_hi), rng.uniform(-2.2, 2.2))
        if chart and k == 0:
            pos = (LAMP_FIRST[0], 0.5 * (y_lo + y_hi), LAMP_FIRST[2])
        tilt, turn = rng.uniform(0.0, 0.35), rng.uniform(0.0, 2 * np.pi)
        colour = rng.uniform(0.4, 1.0, 3)
        inten = (power / n_lamps) * 10.0 ** rng.uniform(-0.5, 0.5)
        spot = spots and (k % 2 == 1 or n_lamps == 1)
        direction = np.array([np.sin(tilt) * np.cos(turn), -np.cos(tilt), np.sin(tilt) * np.sin(turn)])
        lights[k, 0:3], lights[k, 3] = pos, lamp_range
        lights[k, 4:7] = (direction / np.linalg.norm(direction)) if spot else (0, 0, -1)
        lights[k, 7] = 1.0 if spot else 0.0
        lights[k, 8:11] = colour * inten
        lights[k, 11], lights[k, 12] = (np.cos(0.35), np.cos(0.6)) if spot else (1.0, np.cos(np.pi / 4))
    return d, lights


# ---------------------------------------------------------------------------- the corner cluster (deep KD walks)
def _flat_vertices(p):
    """[n, 3, 3] float32 corner positions -> vertices [3 n, 11] (per-triangle normal, tangent along the first edge), triangles [n, 3]."""
    p64 = p.astype(np.float64)
    fn = np.cross(p64[:, 1] - p64[:, 0], p64[:, 2] - p64[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-300)
    tw = p64[:, 1] - p64[:, 0]
    tw /= np.maximum(np.linalg.norm(tw, axis=1, keepdims=True), 1e-300)
    v = np.zeros((3 * len(p), 11), np.float32)
    v[:, 0:3] = p.reshape(-1, 3)
    v[:, 3:5] = np.tile(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (len(p), 1))
    v[:, 5:8] = np.repeat(fn, 3, axis=0)
    v[:, 8:11] = np.repeat(tw, 3, axis=0)
    return v, np.arange(3 * len(p), dtype=np.uint32).reshape(-1, 3)


def corner_cluster(n: int, ratio: float, size: float, scale: float, seed: int = 0):
    """Corner positions [n, 3, 3] float32 of n triangles clustered self-similarly toward the origin: triangle i has
    s_i = scale * ratio**i and corners s_i * (1, 1, 1) + size * s_i * U_i, U_i uniform in [-1, 1]^(3 x 3), drawn in triangle
    order from default_rng(seed); all arithmetic in float32. -> (corners, s [n] float32)"""
    f = np.float32
    rng = np.random.default_rng(seed)
    s = (f(scale) * f(ratio) ** np.arange(n, dtype=np.float32)).astype(np.float32)
    u = rng.uniform(-1.0, 1.0, (n, 3, 3)).astype(np.float32)
    return (s[:, None, None] + f(size) * s[:, None, None] * u).astype(np.float32), s


def corner_cluster_scene(n: int = 60, ratio: float = 0.8, size: float = 0.1, scale: float = 1e3, seed: int = 0, sun: bool = False,
                         surfaces: int = 1, backdrop: int = 0):
    """One model (identity transform) whose surface is a corner_cluster: with the builder's 1e-4 empty-space cuts and child boxes
    that shrink by `ratio`, the SAH tree is a comb that reaches the depth limit, and a ray that starts in the innermost cell and
    runs outwards sets aside one subtree per level (walks with ~20 pending entries; Cornell's rays reach 8).
      surfaces: that many clusters in the one model, surface j drawn with seed + j (all along the same diagonal);
      backdrop: > 0 adds one more surface, a backdrop x backdrop grid across the diagonal beyond the outermost triangle: at 48
                (4608 triangles) it does not fit LDS next to the clusters, so the scene is hybrid-resident.
    The camera sits inside the innermost cell and looks along (1, 1, 1). -> dict of arrays as plaza_scene."""
    f = np.float32
    parts = []
    for j in range(surfaces):
        p, s = corner_cluster(n, ratio, size, scale, seed + j)
        parts.append(_flat_vertices(p))
    if backdrop > 0:
        d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
        ex = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
        ey = np.cross(d, ex)
        half = 1.5 * scale
        gv, gt = _grid(backdrop, 2.0 * scale * np.ones(3) - half * (ex + ey), 2 * half * ey, 2 * half * ex)   # normal towards the origin
        parts.append((gv, gt))
    sr, v0, t0 = [], 0, 0
    for v, t in parts:
        sr.append([v0, len(v), t0, len(t)])
        v0 += len(v); t0 += len(t)
    k = len(parts)
    rng = np.random.default_rng(seed + 1000)
    mats = np.zeros((k, 11), np.float32)
    mats[:, 0:3] = 0.4 + 0.5 * rng.random((k, 3))
    mats[:, 3] = 1.0
    mats[:, 4] = 0.3 + 0.6 * rng.random(k)
    mats[:, 5] = (np.arange(k) % 3) == 1
    mats[:, 9] = 1.45
    eye = (s[-1] * f(1.0 - size) * f(0.5)) * np.ones(3, np.float32)
    cam = np.concatenate([_look_at(eye, eye.astype(np.float64) + 1.0), [f(2.5 * size)]]).astype(np.float32)
    sun13 = None
    if sun:
        dd = np.array([0.2, 0.9, 0.4])
        dd /= np.linalg.norm(dd)
        x = np.cross([0, 1, 0], dd); x /= np.linalg.norm(x)
        sun13 = np.concatenate([x, np.cross(dd, x), dd, [3.0, 2.8, 2.5], [0.004732]]).astype(np.float32)
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    return dict(model_xform=np.array([[0, 0, 0] + ident], np.float32), model_surf=np.array([[0, k]], np.int32),
                surf_range=np.array(sr, np.int32), vertices=np.concatenate([p[0] for p in parts]).astype(np.float32),
                triangles=np.concatenate([p[1] for p in parts]).astype(np.uint32), materials=mats, camera=cam, sun=sun13)


def corner_cluster_rays(n: int, ratio: float, size: float, scale: float, count: int, seed: int = 0, rng_seed: int = 1, corner_f=None,
                        any_cell: bool = False):
    """Rays for corner_cluster_scene(n, ratio, size, scale, seed): origins s_{n-1} * (1 - size) * u, u uniform in [0.2, 1]^3 (inside the
    innermost cell), aimed at a vertex of a random triangle: at vertex * U(0.7, 1.3), or, with corner_f = a list of fractions f, just
    inside the corner: vertex + (centroid - vertex) * f, f cycling through the list. any_cell: the origin scales with a random triangle's
    s_k instead of the innermost one's (walks of every depth up to the deepest). Directions normalised in float32. -> [count, 6]"""
    f = np.float32
    p, s = corner_cluster(n, ratio, size, scale, seed)
    rng = np.random.default_rng(rng_seed)
    cell = rng.integers(0, n, count) if any_cell else np.full(count, n - 1)
    org = (s[cell, None] * f(1.0 - size) * rng.uniform(0.2, 1.0, (count, 3)).astype(np.float32)).astype(np.float32)
    ti, vi = rng.integers(0, n, count), rng.integers(0, 3, count)
    vert = p[ti, vi]
    if corner_f is None:
        tgt = vert * rng.uniform(0.7, 1.3, (count, 3)).astype(np.float32)
    else:
        cen = p[ti].mean(1, dtype=np.float32)
        fr = np.asarray(corner_f, np.float32)[np.arange(count) % len(corner_f)]
        tgt = vert + (cen - vert) * fr[:, None]
    d = (tgt - org).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return np.concatenate([org, d], 1).astype(np.float32)


def _box(half):
    """Axis-aligned box of half-extents `half` ([3] or a scalar) around the origin: 24 vertices (flat normals), 12 triangles, outward."""
    h = np.broadcast_to(np.asarray(half, np.float64), (3,))
    v, t = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            n = np.zeros(3); n[axis] = sign
            ta = np.zeros(3); ta[a] = 1.0
            base = len(v)
            for k, (sa, sb) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
                p = np.zeros(3)
                p[axis], p[a], p[b] = sign * h[axis], sa * h[a], sb * h[b]
                v.append(np.concatenate([p, [(sa + 1) / 2, (sb + 1) / 2], n, ta]))
            t += [[base, base + 1, base + 2], [base, base + 2, base + 3]] if sign > 0 else [[base, base + 2, base + 1], [base, base + 3, base + 2]]
    return np.array(v, np.float32), np.array(t, np.uint32)


def _xform(origin, rot_y_deg=0.0, scale=1.0):
    """[12] float32: origin, basis columns of scale * R_y(angle)."""
    a = np.deg2rad(rot_y_deg)
    c, s = np.cos(a), np.sin(a)
    basis = scale * np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)   # rows; columns are the images of x, y, z
    return np.concatenate([np.asarray(origin, np.float64), basis.T.ravel()]).astype(np.float32)


def movers_scene(emissive_mover: bool = False, sun: bool = False, alpha: bool = False):
    """The motion-blur test scene: few surfaces and a few hundred triangles, so that every intersect route takes it. Static floor and static
    emissive quad; a translating box; an icosphere(2) that rotates 20 degrees about y and scales 1 -> 1.2; a two-surface model that moves;
    two boxes whose current transforms are bitwise equal and whose begin transforms differ; two boxes equal in both keys; with
    `emissive_mover` one emissive box that moves. `sun` adds a directional light, `alpha` makes the second surface of the two-surface model
    half-transparent. -> the arrays of plaza_scene plus begin_model_xform [n,12] (the state at u = 0; model_xform is the state at u = 1) and
    begin_camera [13] (camera is the state at u = 1): keys a few degrees and a few centimetres apart."""
    ident = _xform([0, 0, 0])
    meshes, models = [], []   # (vertices, triangles, material) ; (first surface, count, begin xform, current xform)

    def add(parts, begin, cur):
        models.append((len(meshes), len(parts), np.asarray(begin, np.float32), np.asarray(cur, np.float32)))
        meshes.extend(parts)

    def mat(albedo, rough=0.6, metal=0.0, emissive=(0, 0, 0), opacity=1.0):
        return np.array(list(albedo) + [opacity, rough, metal] + list(emissive) + [1.33, 0.0], np.float32)

    fv, ft = _quad(0.0, 4.0)
    add([(fv, ft, mat((0.7, 0.7, 0.7)))], ident, ident)                                            # 0 static floor
    lv, lt = _quad(0.0, 0.6)
    lamp = np.array([0.2, 2.6, 0.1, 1, 0, 0, 0, -1, 0, 0, 0, -1], np.float32)                      # half-turn about x: the quad faces down (-0.0 entries stay)
    lamp[[4, 5, 6, 8, 9, 10]] = [0.0, 0.0, -0.0, -0.0, 0.0, -0.0]
    add([(lv, lt, mat((0.8, 0.8, 0.8), emissive=(1.7, 1.5, 1.2)))], lamp, lamp)                    # 1 static emissive quad
    bv, bt = _box(0.4)
    add([(bv, bt, mat((0.8, 0.3, 0.25)))], _xform([-1.5, 0.4, 0.0]), _xform([-1.1, 0.4, 0.3]))     # 2 translating box
    sv, st = icosphere(2)
    s11 = np.zeros((len(sv), 11), np.float32)
    s11[:, 0:3] = sv
    s11[:, 3] = np.arctan2(sv[:, 2], sv[:, 0]) / (2 * np.pi) + 0.5
    s11[:, 4] = np.arcsin(np.clip(sv[:, 1], -1, 1)) / np.pi + 0.5
    s11[:, 5:8] = sv
    tan = np.cross(np.where(np.abs(sv[:, 1:2]) < 0.99, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]]), sv)
    s11[:, 8:11] = tan / np.linalg.norm(tan, axis=1, keepdims=True)
    add([(s11, st.astype(np.uint32), mat((0.3, 0.5, 0.85), rough=0.3, metal=0.6))],
        _xform([0.2, 0.6, -0.5], 0.0, 0.5), _xform([0.2, 0.6, -0.5], 20.0, 0.6))                   # 3 rotating, growing sphere
    tv, tt = _box([0.3, 0.2, 0.3])
    qv, qt = _quad(0.45, 0.35)
    add([(tv, tt, mat((0.35, 0.75, 0.4))), (qv, qt, mat((0.9, 0.85, 0.3), opacity=0.5 if alpha else 1.0))],
        _xform([1.2, 0.2, -0.9], -6.0), _xform([1.35, 0.25, -0.8], 4.0))                           # 4 two-surface model that moves
    av, at = _box(0.3)
    cv, ct = _box([0.2, 0.45, 0.2])
    meet = _xform([1.3, 0.45, 0.8], 10.0)
    add([(av, at, mat((0.75, 0.6, 0.3)))], _xform([1.0, 0.45, 0.6], 0.0), meet)                     # 5, 6 meet at u = 1 from different begin states
    add([(cv, ct, mat((0.3, 0.6, 0.75)))], _xform([1.5, 0.6, 1.1], 25.0), meet)
    dv, dt = _box([0.25, 0.25, 0.25])
    ev, et = _box([0.15, 0.4, 0.15])
    pair_a, pair_b = _xform([-0.9, 0.4, 1.2], -8.0), _xform([-0.7, 0.4, 1.35], 5.0)
    add([(dv, dt, mat((0.6, 0.3, 0.7)))], pair_a, pair_b)                                           # 7, 8 equal in both keys: one moving ray space
    add([(ev, et, mat((0.7, 0.7, 0.3)))], pair_a, pair_b)
    if emissive_mover:
        gv, gt = _box(0.2)
        add([(gv, gt, mat((0.8, 0.8, 0.8), emissive=(0.9, 1.1, 1.4)))], _xform([-0.3, 1.5, 0.9]), _xform([0.0, 1.6, 0.8], 12.0))   # 9 moving emitter
    verts, tris, sr, mats = [], [], [], []
    nv = nt = 0
    for v, t, m in meshes:
        sr.append([nv, len(v), nt, len(t)])
        verts.append(v); tris.append(t); mats.append(m)
        nv += len(v); nt += len(t)
    cam_end = np.concatenate([_look_at([0.3, 2.1, 5.2], [0.1, 0.6, 0.0]), [np.float32(0.75)]]).astype(np.float32)
    cam_begin = np.concatenate([_look_at([0.22, 2.13, 5.25], [0.0, 0.62, 0.0]), [np.float32(0.75)]]).astype(np.float32)
    sun13 = None
    if sun:
        d = np.array([0.4, 0.75, 0.5])
        d /= np.linalg.norm(d)
        x = np.cross([0, 1, 0], d)
        x /= np.linalg.norm(x)
        sun13 = np.concatenate([x, np.cross(d, x), d, [2.5, 2.3, 2.0], [0.004732]]).astype(np.float32)
    return dict(model_xform=np.stack([m[3] for m in models]), begin_model_xform=np.stack([m[2] for m in models]),
                model_surf=np.array([[m[0], m[1]] for m in models], np.int32), surf_range=np.array(sr, np.int32),
                vertices=np.concatenate(verts).astype(np.float32), triangles=np.concatenate(tris).astype(np.uint32),
                materials=np.stack(mats), camera=cam_end, begin_camera=cam_begin, sun=sun13)


# ---------------------------------------------------------------------------- the emitter field (many small emissive quads)
def emitter_field_scene(n: int = 16, seed: int = 7):
    """A diffuse floor (8 x 8 on y = 0) seen from above at an angle, lit by `n` small emissive quads facing down, for the light tree of
    ptx_render_nee (Scene.set_light_pick): the list has 2 n triangles whose distances from a shading point differ by an order of magnitude.
      emitters: on a jittered ceil(sqrt(n))^2 grid over |x|, |z| < 3.4, at heights 0.35 .. 1.6, half sizes 0.04 .. 0.12; emitter k belongs
                to surface 4 + k % min(n, 8), and each of those surfaces has its own emissive factor (log-uniform over a decade), so powers
                vary through both the area and the factor.
      blockers: three opaque quads at y = 0.25, 0.2 and 0.3 (surfaces 1 .. 3).
      No sun, no alpha, no textures. One model; small n keeps the scene on the LDS route.
    -> dict of arrays as plaza_scene, plus `emitters` [n, 5]: centre x, y, z, half size, surface."""
    rng = np.random.default_rng(seed)
    n_es = min(n, 8)
    surf_v = [[] for _ in range(4 + n_es)]   # per surface: its quads' vertex blocks
    mats = [None] * (4 + n_es)

    def add(s, x0, x1, z0, z1, y, up):
        v = np.zeros((4, 11), np.float32)
        v[:, 0:3] = [[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]]
        v[:, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
        v[:, 5:8] = [0, 1 if up else -1, 0]
        v[:, 8:11] = [1, 0, 0]
        surf_v[s].append((v, up))
    add(0, -4, 4, -4, 4, 0.0, True)
    mats[0] = [0.7, 0.7, 0.7, 1.0, 0.6, 0.0, 0, 0, 0, 1.33, 0]
    for s, (x0, x1, z0, z1, y) in enumerate([(-2.6, -1.2, -0.4, 0.9, 0.25), (0.6, 2.2, -2.4, -1.3, 0.2), (0.9, 2.0, 1.2, 2.6, 0.3)], 1):
        add(s, x0, x1, z0, z1, y, True)
        mats[s] = [0.4, 0.5, 0.6, 1.0, 0.5, 0.0, 0, 0, 0, 1.33, 0]
    for j in range(n_es):
        colour = rng.uniform(0.5, 1.0, 3)
        mats[4 + j] = [0.8, 0.8, 0.8, 1.0, 0.5, 0.0] + list(colour * 4.0 * 10.0 ** rng.uniform(-0.5, 0.5)) + [1.33, 0]
    side = int(np.ceil(np.sqrt(n)))
    cell = 6.8 / side
    emitters = np.zeros((n, 5), np.float32)
    for k in range(n):
        cx = -3.4 + (k % side + rng.uniform(0.25, 0.75)) * cell
        cz = -3.4 + (k // side + rng.uniform(0.25, 0.75)) * cell
        y, hs = rng.uniform(0.35, 1.6), rng.uniform(0.04, 0.12)
        add(4 + k % n_es, cx - hs, cx + hs, cz - hs, cz + hs, y, False)
        emitters[k] = [cx, y, cz, hs, 4 + k % n_es]
    verts, tris, ranges = [], [], []
    nv = nt = 0
    for quads in surf_v:
        ranges.append([nv, 4 * len(quads), nt, 2 * len(quads)])
        for q, (v, up) in enumerate(quads):
            verts.append(v)
            local = np.array([[0, 2, 1], [0, 3, 2]] if up else [[0, 1, 2], [0, 2, 3]], np.uint32) + np.uint32(4 * q)
            tris.append(local)
        nv += 4 * len(quads)
        nt += 2 * len(quads)
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    cam = np.concatenate([_look_at([0.0, 5.0, 4.5], [0.0, 0.0, 0.0]), [np.float32(0.8)]]).astype(np.float32)
    return dict(model_xform=np.array([[0, 0, 0] + ident], np.float32), model_surf=np.array([[0, len(surf_v)]], np.int32),
                surf_range=np.array(ranges, np.int32), vertices=np.concatenate(verts), triangles=np.concatenate(tris),
                materials=np.array(mats, np.float32), camera=cam, sun=None, emitters=emitters)
