"""tests/_routes.py itself, without a GPU and without the product: the route tables, the switches a route leaves in the environment, and
the scene cache's handling of PTX_FORCE_GLOBAL."""
import os

import pytest

from _routes import DEFAULT_ROUTES, ROUTE_VARS, Route, Scenes, forced_routes, route_named, use_route


def test_forced_routes_at_the_64_surface_limit():
    for n_surf, name, pipeline in ((64, "queue", 1), (65, "queue refused", 0)):
        routes = forced_routes(n_surf)
        assert [r.name for r in routes[:2]] == ["lds fused", "global fused"]
        assert (routes[2].name, routes[2].pipeline) == (name, pipeline)
        assert routes[2].force_global and routes[2].resident == 0 and routes[2].env == {"PTX_WAVEFRONT": "1"}
        assert all(r.env["PTX_WAVEFRONT"] in ("0", "1") and set(r.env) == {"PTX_WAVEFRONT"} for r in routes)     # forced: never the product's choice
    # the default-choice family leaves "lds fused" and "queue" to the product
    assert route_named(DEFAULT_ROUTES, "lds fused").env == {} and route_named(DEFAULT_ROUTES, "queue").env == {}
    assert route_named(DEFAULT_ROUTES, "global fused").env == {"PTX_WAVEFRONT": "0"}


def test_use_route_sets_exactly_the_routes_switches(monkeypatch):
    monkeypatch.setenv("PTX_WF_PAIRS_M", "1")                # a stray switch of an earlier route
    monkeypatch.setenv("PTX_WAVEFRONT", "1")
    use_route(monkeypatch, Route("r", False, {"PTX_WAVEFRONT": "0", "PTX_SURFACE_UNITS": "1"}, 1, 0))
    assert {k: os.environ[k] for k in ROUTE_VARS if k in os.environ} == {"PTX_WAVEFRONT": "0", "PTX_SURFACE_UNITS": "1"}
    use_route(monkeypatch, Route("r", False, {}, 1, 0))
    assert not [k for k in ROUTE_VARS if k in os.environ]


def test_scene_cache_is_lazy_keyed_and_unsets_the_switch(monkeypatch):
    monkeypatch.delenv("PTX_FORCE_GLOBAL", raising=False)
    made = []

    def make(ptx, ctx, name):
        if name == "broken":
            raise RuntimeError("no such scene")
        made.append((name, os.environ.get("PTX_FORCE_GLOBAL")))
        return object()
    scenes = Scenes(make)
    assert made == []                                        # nothing is created up front
    a = scenes.get(None, None, monkeypatch, "a")
    g = scenes.get(None, None, monkeypatch, "a", True)
    assert made == [("a", None), ("a", "1")] and a is not g and "PTX_FORCE_GLOBAL" not in os.environ
    assert scenes.get(None, None, monkeypatch, "a") is a and scenes.get(None, None, monkeypatch, "a", True) is g and len(made) == 2
    with pytest.raises(RuntimeError):
        scenes.get(None, None, monkeypatch, "broken", True)
    assert "PTX_FORCE_GLOBAL" not in os.environ              # unset after a make that raises
    assert Scenes(make).get(None, None, monkeypatch, "a") is not a     # another module's instance shares nothing
