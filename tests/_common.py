"""The three one-liners nearly every test file needs. Not collected (underscore prefix); import by name."""
import importlib

import numpy as np


def _proc():
    return importlib.import_module("distributed-path-tracer_amd.procedural")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


proc, bits, same = _proc, _bits, _same    # the test files keep the underscore names their bodies were written with
