"""numpy restatement of the stored CDF of ptx_render_nee's punctual lights (include/ptx.h: PUNCTUAL LIGHTS, ptx_scene_set_punctual_lights), for
tests/_nee_estimator.py, tests/test_nee_punctual.py and tests/test_nee_punctual_gpu.py; the third kind of candidate is in
tests/_nee_estimator.py (punctual).

cdf_of: the CDF as ptx_scene_set_punctual_lights builds it.
"""
import numpy as np

f32 = np.float32


def cdf_of(lights):
    """[n, 16] records -> the stored CDF [n] float32 (float64 shares of lum(intensity), the last entry 1), or None when there is no light or
    every light is black: ptx_scene_set_punctual_lights then stores none"""
    if lights is None or len(lights) == 0:
        return None
    I = np.asarray(lights, f32).reshape(-1, 16)[:, 8:11].astype(np.float64)
    cum = np.cumsum((0.2126 * I[:, 0] + 0.7152 * I[:, 1]) + 0.0722 * I[:, 2])
    if not cum[-1] > 0:
        return None
    cdf = (cum / cum[-1]).astype(f32)
    cdf[-1] = 1
    return cdf
