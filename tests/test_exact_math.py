"""The short reciprocal / square-root sequences the kernels use in place of LLVM's IEEE ones (csrc/device_core.hpp: rcp_exact — the
triangle test's reciprocal with its range test and fallback —, sqrt_exact, rsqrt_exact), run on the device as compiled into the
library, against the IEEE expressions 1.0f / x, sqrtf(x), 1.0f / sqrtf(x) for every one of the 2^32 float patterns. A result counts
as a mismatch when its bits differ (any NaN equals any NaN)."""
import pytest


@pytest.mark.gpu
def test_short_sequences_match_ieee_for_every_float(ptx):
    ctx = ptx.Context(0)
    bad = ctx.exact_math_check()
    assert set(bad) == {"rcp", "sqrt", "rsqrt"}
    assert bad == {k: 0 for k in bad}, bad
