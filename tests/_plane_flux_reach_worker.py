"""Worker of tests/test_gpu_plane_flux.py: the three steps of its reach-mask test in a process of its own, so that the environment
(ASORA_REACH_MASK, read once per process) decides about the mask.
    python _plane_flux_reach_worker.py out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pyc2ray_amd as p
    import test_gpu_plane_flux as T
    res = {"mode": os.environ.get("ASORA_REACH_MASK", "")}
    for k, (niter, x, phi) in enumerate(T.reach_mask_steps(p)):
        res.update({f"niter{k}": niter, f"xh{k}": x, f"phi{k}": phi})
    np.savez(sys.argv[1], **res)
    p.device_close()


if __name__ == "__main__":
    main()
