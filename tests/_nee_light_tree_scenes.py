"""The scenes of tests/test_nee_light_tree.py and tests/test_nee_light_tree_gpu.py: lists of a few emissive triangles laid out by hand (one,
two, three, coincident centroids, centroids on one line, four large emitters over a glossy floor), procedural.emitter_field_scene and
emitter_cloud_scene, each with its oracle, light list and restated tree, built once. Not collected (underscore prefix)."""
import numpy as np

import _nee_light_tree_restatement as LT
from _common import _proc
from _nee_common import _oracle
from _nee_restatement import light_list
from conftest import CORNELL, oracle_from_dict, product_from_dict

f32 = np.float32


# ---------------------------------------------------------------------------- scenes
def tri_scene(corners, factors=((2.0, 1.5, 1.0),), per_surface=None):
    """a floor and emissive triangles with the given world corners [n, 3, 3]; triangle k belongs to emissive surface k % len(factors)"""
    corners = np.asarray(corners, np.float64).reshape(-1, 3, 3)
    n_es = len(factors)
    groups = [[k for k in range(len(corners)) if k % n_es == j] for j in range(n_es)]
    groups = [g for g in groups if g]
    verts, tris, ranges, mats = [], [], [], []
    v = np.zeros((4, 11), f32)
    v[:, 0:3] = [[-4, 0, -4], [4, 0, -4], [4, 0, 4], [-4, 0, 4]]
    v[:, 3:5], v[:, 5:8], v[:, 8:11] = [[0, 0], [1, 0], [1, 1], [0, 1]], [0, 1, 0], [1, 0, 0]
    verts.append(v)
    tris.append(np.array([[0, 2, 1], [0, 3, 2]], np.uint32))
    ranges.append([0, 4, 0, 2])
    mats.append([0.7, 0.7, 0.7, 1.0, 0.6, 0.0, 0, 0, 0, 1.33, 0])
    nv, nt = 4, 2
    for j, g in enumerate(groups):
        ranges.append([nv, 3 * len(g), nt, len(g)])
        for q, k in enumerate(g):
            c = corners[k]
            nrm = np.cross(c[1] - c[0], c[2] - c[0])
            ln = np.linalg.norm(nrm)
            nrm = nrm / ln if ln > 0 else np.array([0.0, -1.0, 0.0])
            tan = c[1] - c[0]
            tl = np.linalg.norm(tan)
            tan = tan / tl if tl > 0 else np.array([1.0, 0.0, 0.0])
            vv = np.zeros((3, 11), f32)
            vv[:, 0:3], vv[:, 3:5], vv[:, 5:8], vv[:, 8:11] = c, [[0, 0], [1, 0], [0, 1]], nrm, tan
            verts.append(vv)
            tris.append(np.array([[3 * q, 3 * q + 1, 3 * q + 2]], np.uint32))
        nv += 3 * len(g)
        nt += len(g)
        mats.append([0.8, 0.8, 0.8, 1.0, 0.5, 0.0, *factors[j], 1.33, 0])
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    P = _proc()
    cam = np.concatenate([P._look_at([0.0, 5.0, 4.5], [0.0, 0.0, 0.0]), [f32(0.8)]]).astype(f32)
    return dict(model_xform=np.array([[0, 0, 0] + ident], f32), model_surf=np.array([[0, len(ranges)]], np.int32),
                surf_range=np.array(ranges, np.int32), vertices=np.concatenate(verts), triangles=np.concatenate(tris),
                materials=np.array(mats, f32), camera=cam, sun=None)


def _down_tri(cx, cy, cz, r, turn=0.0):
    """a triangle facing down, centroid (cx, cy, cz), circumradius r"""
    a = turn + np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])
    return np.stack([cx + r * np.cos(a), np.full(3, cy), cz + r * np.sin(a)], 1)


def _special(name):
    rng = np.random.default_rng(5)
    if name == "1 triangle":
        return tri_scene([_down_tri(0.3, 1.5, -0.2, 0.2)])
    if name in ("2 triangles", "3 triangles"):
        n = int(name[0])
        return tri_scene([_down_tri(rng.uniform(-2, 2), rng.uniform(0.5, 2), rng.uniform(-2, 2), rng.uniform(0.05, 0.3)) for _ in range(n)],
                         factors=((2.0, 1.5, 1.0), (0.2, 0.3, 0.9)))
    if name == "coincident centroids":      # six triangles about one centroid, of different sizes and turns
        return tri_scene([_down_tri(1.0, 2.0, 0.5, 0.1 + 0.05 * k, 0.3 * k) for k in range(6)], factors=((2.0, 1.5, 1.0), (0.5, 0.5, 2.0)))
    if name == "centroids on one line":     # ties along x, to be broken by the index
        xs = [0.5, -1.0, 0.5, 2.0, -1.0, 0.25, 0.5]
        return tri_scene([_down_tri(x, 2.0, 0.0, 0.15, 0.2 * k) for k, x in enumerate(xs)])
    if name == "gloss4":                    # four large emitters well above a glossy metallic floor: a BSDF sample from a floor point hits an
        d = tri_scene([_down_tri(x, y, z, r, t) for x, y, z, r, t in [(-1.6, 2.5, -1.2, 1.0, 0.0), (1.5, 2.8, -1.0, 0.8, 0.4), (-1.2, 2.2, 1.4, 0.9, 0.9),
                                                                      (1.4, 2.4, 1.5, 0.7, 1.3)]], factors=((0.2, 0.15, 0.1), (0.05, 0.1, 0.2)))
        d["materials"][0, 4:6] = [0.2, 0.9]  # emitter far from it often, and with a large weight: the emission weight carries the frame
        return d
    raise KeyError(name)


_dicts = {}


def scene_dict(name):
    if name not in _dicts:
        P = _proc()
        if name.startswith("field"):
            _dicts[name] = P.emitter_field_scene(int(name[5:]))
        elif name == "cloud":
            _dicts[name] = P.emitter_cloud_scene()
        else:
            _dicts[name] = _special(name)
    return _dicts[name]


TREE_CASES = {"1 triangle": 1, "2 triangles": 2, "3 triangles": 3, "field32": 64, "cloud": 271, "coincident centroids": 6, "centroids on one line": 7}
_trees = {}


def restated(ora, name):
    """(oracle scene, arrays, light list, tree, path) of a case, built once"""
    if name not in _trees:
        if name == "cornell":
            o, a = _oracle(ora, "cornell")
        else:
            o = oracle_from_dict(ora, scene_dict(name))
            a = o.a
        ll = light_list(a)
        T, path = LT.build(a, ll)
        for v in (T, path):
            v.setflags(write=False)
        _trees[name] = (o, a, ll, T, path)
    return _trees[name]


def host_scene(ptx, name, tree=True):
    s = ptx.Scene.load_gltf(None, CORNELL) if name == "cornell" else product_from_dict(ptx, None, scene_dict(name))
    if tree:
        s.set_light_pick("tree")
    return s
