"""GPU: per-source spectra across ranks -- evolve3D_MPI(src_spectrum=...) on two gloo ranks that share the GPU, through the slab
exchange (sources re-ordered by their first coordinate and cut into shards) and the all-reduce loop (contiguous shards): each
rank's shard of the sources must take its shard of the spectra."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


@pytest.fixture(scope="module")
def single():
    """The one-GPU evolve3D of the workers' case, with and without the spectra: computed once for both exchanges."""
    import pyc2ray_amd as p
    import pyc2ray_amd.evolve as ev
    import _spectra_dist_worker as W
    c = W.case()
    if p.cuda_is_init():
        p.device_close()
    p.device_init(c["N"], 8)
    p.spectra_to_device(*c["spectra"])
    with_spectra = W.evolve(p, ev, c)
    without = W.evolve(p, ev, c, spectrum=False)
    p.device_close()
    assert not np.allclose(with_spectra[1], without[1], rtol=1e-3, atol=0)      # the spectra matter in this case
    assert 0 < c["spec"].sum() < c["spec"].shape[0]
    return with_spectra


@pytest.mark.parametrize("exchange", ["slab", "allreduce"])
def test_two_ranks_with_two_spectra(single, tmp_path, exchange):
    """24^3, 37 sources, two table sets: equal iteration counts, grids bit-identical between the ranks and equal to the one-GPU
    evolve3D to 1e-10."""
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, PYC2RAY_AMD_NO_TORCH="0", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_spectra_dist_worker.py"), str(r), str(world), port, outs[r],
                               exchange], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [q.communicate(timeout=300)[0].decode() for q in procs]
    for q, log in zip(procs, logs):
        assert q.returncode == 0, log
    res = [np.load(o) for o in outs]
    assert np.array_equal(res[0]["xh"], res[1]["xh"]) and np.array_equal(res[0]["phi"], res[1]["phi"])
    assert int(res[0]["niter"]) == int(res[1]["niter"]) == single[2]
    np.testing.assert_allclose(res[0]["xh"], single[0], rtol=1e-10, atol=0)
    np.testing.assert_allclose(res[0]["phi"], single[1], rtol=1e-10, atol=0)
