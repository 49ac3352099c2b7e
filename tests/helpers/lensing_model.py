"""The HaloModel the GPU lensing tests share (tests/test_gpu_lensing.py, tests/test_gpu_delta_sigma.py)."""
import numpy as np


def model(zs, ks=None, ms=None):
    import hmvec_amd as hm
    ks = np.geomspace(1e-4, 100, 200) if ks is None else ks
    ms = np.geomspace(2e10, 1e17, 40) if ms is None else ms
    return hm.HaloModel(np.atleast_1d(zs), ks, ms=ms, accuracy="low", engine="analytic")
