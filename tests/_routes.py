"""The route harness of the GPU tests, stated once.

A route is a way the product can take a scene through a render or a batch of intersections: the fused kernel on LDS-resident geometry,
the fused kernel on global memory (the scene created under PTX_FORCE_GLOBAL), the queue pipeline. A test walks the routes, and each route
is asserted from the scene's residency (info()["lds_resident"]) and from the pipeline the context reports (timing()["pipeline"]), so that a
silent fallback cannot pass.

Two families of routes exist and stay apart, because they test different things:
  * forced_routes(n_surf): PTX_WAVEFRONT is "0" or "1" on every route; above 64 surfaces the queue pipeline must refuse.
  * DEFAULT_ROUTES: "lds fused" and "queue" run with no switch at the call, so the product's own pipeline choice is what is tested.
Tables of one scene per entry (tests/test_aov.py, tests/test_adaptive.py) are lists of Route records in their own files.

This module is not collected (underscore prefix). The fixtures `clean_env` and `ctx` are imported by name into a test module; an imported
fixture belongs to the importing module, so every module has its own context. Pytest does not rewrite asserts here: each carries its message.
"""
import collections

import pytest

ROUTE_VARS = ("PTX_WAVEFRONT", "PTX_FORCE_GLOBAL", "PTX_SURFACE_UNITS", "PTX_NO_HYBRID", "PTX_WF_PAIRS_M", "PTX_WF_RATIO_GUESS")

# name; whether the scene is created under PTX_FORCE_GLOBAL; the switches set at the call; the expected lds_resident and pipeline
Route = collections.namedtuple("Route", "name force_global env resident pipeline")


@pytest.fixture
def clean_env(monkeypatch):
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def ctx(ptx):
    return ptx.Context(0)


def forced_routes(n_surf):
    r = [Route("lds fused", False, {"PTX_WAVEFRONT": "0"}, 1, 0), Route("global fused", True, {"PTX_WAVEFRONT": "0"}, 0, 0)]
    # the queue pipeline takes at most 64 surfaces: above that PTX_WAVEFRONT=1 must leave the fused kernel in charge
    r.append(Route("queue", True, {"PTX_WAVEFRONT": "1"}, 0, 1) if n_surf <= 64 else Route("queue refused", True, {"PTX_WAVEFRONT": "1"}, 0, 0))
    return r


DEFAULT_ROUTES = [Route("lds fused", False, {}, 1, 0), Route("queue", True, {}, 0, 1), Route("global fused", True, {"PTX_WAVEFRONT": "0"}, 0, 0)]


def route_named(routes, name):
    return next(r for r in routes if r.name == name)


def under_force_global(mp, force_global, create):
    """create() with PTX_FORCE_GLOBAL set if asked for; the switch is unset afterwards, also when create() raises."""
    if force_global:
        mp.setenv("PTX_FORCE_GLOBAL", "1")
    try:
        return create()
    finally:
        mp.delenv("PTX_FORCE_GLOBAL", raising=False)


class Scenes:
    """A test module's scenes: make(ptx, ctx, name), created on first use and kept by (name, force_global). One instance per module: a scene
    lives on the context it was created on, whose timing() the module's tests read, so instances are never shared between modules."""

    def __init__(self, make):
        self._make, self._kept = make, {}

    def get(self, ptx, ctx, mp, name, force_global=False):
        if (name, force_global) not in self._kept:
            self._kept[(name, force_global)] = under_force_global(mp, force_global, lambda: self._make(ptx, ctx, name))
        return self._kept[(name, force_global)]


def use_route(mp, route):
    for k in ROUTE_VARS:
        mp.delenv(k, raising=False)
    for k, v in route.env.items():
        mp.setenv(k, v)


def resident_as_listed(route, resident):
    return resident == route.resident


def resident_by_creation(route, resident):
    """for scenes whose default residency is not known to the route table: 0 under PTX_FORCE_GLOBAL, all or part of the geometry in LDS without"""
    return resident == 0 if route.force_global else resident in (1, 2)


def on_route(scenes, ptx, ctx, mp, name, route, resident_ok=resident_as_listed):
    """The scene of `name` for the route, with the route's switches set and its residency asserted; the call sites assert the pipeline. The
    scene is taken (and, the first time, created) before the switches of the route are set."""
    s = scenes.get(ptx, ctx, mp, name, route.force_global)
    use_route(mp, route)
    resident = s.info()["lds_resident"]
    assert resident_ok(route, resident), (name, route.name, resident)
    return s


def each_route(scenes, ptx, ctx, mp, name, routes=DEFAULT_ROUTES, resident_ok=resident_as_listed):
    """(route, scene) per route, as on_route gives it"""
    for route in routes:
        yield route, on_route(scenes, ptx, ctx, mp, name, route, resident_ok)


def assert_route(ctx, s, route, what):
    """Residency from info(); the pipeline from a tiny ptx_render under the same environment (ptx_intersect_batch, ptx_render_aov and
    ptx_render_adaptive route their rays with ptx_render's rule)."""
    resident = s.info()["lds_resident"]
    assert resident == route.resident, (what, resident, route.resident)
    s.render(32, 18, 1, 2)
    pipeline = ctx.timing()["pipeline"]
    assert pipeline == route.pipeline, (what, pipeline, route.pipeline)
