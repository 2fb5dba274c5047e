"""numpy restatement of PTX_NEE_SAMPLER_PDF's density (include/ptx.h: THE DENSITY), for tests/_nee_estimator.py and tests/test_nee_sampler_pdf.py;
where ps takes pe's place is in tests/_nee_estimator.py (spdf).

sampler_pdf: the density on float32 arrays in the specification's operation order; ps_diff is the oracle's pdf_diffuse.
ggx_density: ps_spec alone, for the checks of the density against the oracle's importance_specular draws.
"""
import numpy as np

from _nee_restatement import _dot, _lerp, _pbr, f32


def ggx_density(normal, outc, w, rough):
    """ps_spec [n]: the density of importance_specular's direction w (rough: after max(roughness, 0.05F)). The arithmetic is that of the
    arguments' type: float32 arrays restate the product, float64 arrays give the formula itself (the quadrature of the density test)."""
    t_ = normal.dtype.type
    with np.errstate(all="ignore"):
        a = rough * rough
        a2 = a * a
        hv = outc + w
        h = hv / np.sqrt(_dot(hv, hv))[:, None]
        nh, oh = _dot(normal, h), _dot(outc, h)
        t = (nh * nh) * (a2 - t_(1)) + t_(1)
        ps = (a2 * nh) / (((t_(np.pi) * t) * t) * (t_(4) * oh))
    return np.where((nh > 0) & (oh > 0), ps, t_(0)).astype(t_)


def sampler_pdf(ora, normal, outc, w, rough, spec_prob, ior):
    """ps [n] float32 = lerpf(pdf_diffuse(normal, w), ps_spec, spec_prob)"""
    dpdf = _pbr(ora, normal, outc, w, 0, 0, rough, 1, ior)[:, 9]
    return _lerp(dpdf, ggx_density(normal, outc, w, rough), spec_prob).astype(f32)
