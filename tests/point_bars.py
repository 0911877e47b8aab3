"""Float-ulp bars on float32 points against a reference (shared by the GPU tests that hold kernels to the last bits)."""
import numpy as np


def scaled_ulps(got, ref):
    """Per coordinate: |got - ref| in float32 ulps of max(|ref_i|, 2^-6 * |ref|)."""
    r = ref.astype(np.float64)
    scale = np.maximum(np.abs(r), 2.0 ** -6 * np.linalg.norm(r, axis=-1, keepdims=True))
    return np.abs(got.astype(np.float64) - r) / np.spacing(scale.astype(np.float32)).astype(np.float64)


def exact_fraction(got, ref):
    return float(np.mean((got.view(np.uint32) == ref.view(np.uint32)).all(-1)))
