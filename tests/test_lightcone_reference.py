"""CPU: properties of the numpy statement of the light cone (tests/lightcone_reference.py) and of the slices' redshifts
(pyc2ray_amd.lightcone.slice_redshifts): what the device tests then hold the library to."""
import numpy as np
import pytest

import lightcone_reference as R

EPS = float(np.finfo(np.float64).eps)


def _cosmology():
    from pyc2ray_amd.c2ray_base import FlatLambdaCDMLite
    return FlatLambdaCDMLite(70.0, 0.27, 2.726, Ob0=0.044)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_weights_one_and_zero_return_the_planes(axis):
    N = 9
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N)) * 1e300
    planes = [4, 0, 8, 4]
    ones, zeros = np.ones(len(planes)), np.zeros(len(planes))
    prev = R.blend(a, b, planes, ones, zeros, axis)
    now = R.blend(a, b, planes, zeros, ones, axis)
    for t, p in enumerate(planes):
        assert prev[t].tobytes() == np.ascontiguousarray(np.take(a, p, axis=axis)).tobytes()
        assert now[t].tobytes() == np.ascontiguousarray(np.take(b, p, axis=axis)).tobytes()
    # the two remaining axes in ascending order: out[t][a][b]
    idx = [1, 2]
    idx.insert(axis, planes[0])
    assert prev[0][1, 2] == a[tuple(idx)]


def test_the_kinds():
    x, n, T = R.fields(6, 1)
    nbar = float(np.mean(n))
    assert R.form(R.XH, x, n, T, nbar).tobytes() == x.tobytes()
    assert np.array_equal(R.form(R.XHI, x, n, T, nbar), 1.0 - x)
    assert np.array_equal(R.form(R.DENSITY, x, n, T, nbar), n / nbar)
    hi = R.form(R.HI, x, n, T, nbar)
    assert np.array_equal(hi, (1.0 - x) * (n / nbar)) and np.all(hi[x == 1.0] == 0.0)
    assert np.array_equal(R.form(R.HI, x, n, T, nbar, 27.0), hi * (1.0 - 27.0 / T))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_field_linear_in_z_is_reproduced(seed):
    """Every cell a + b z at the states' redshifts: the cone holds a + b z_m, however the steps are placed.  The bound: the two
    fields carry 2 u G each (G = |a| + |b| z, u = eps / 2), f three roundings that weigh on b (z_prev - z_now) only, 1 - f one, the
    two products one each and the sum one: 8 u G = 4 eps G."""
    rng = np.random.default_rng(seed)
    N, a, b = 5, float(rng.uniform(-3, 3)), float(rng.uniform(-2, 2))
    z_states = np.sort(rng.uniform(6.0, 9.0, 7))[::-1]
    z_states = np.r_[z_states, z_states[-1] - 1e-9]                       # (a step that crosses nothing)
    z_slices = np.sort(rng.uniform(z_states[-1], z_states[0], 40))[::-1]
    fields = [np.full((N, N, N), a + b * z) for z in z_states]
    cube, emitted_by = R.build_cone(fields, z_states, z_slices, first_plane=2, axis=seed)
    assert cube.shape == (40, N, N) and len(emitted_by) == 40
    exact = np.array([np.longdouble(a) + np.longdouble(b) * np.longdouble(z) for z in z_slices])
    err = np.max(np.abs(cube.astype(np.longdouble) - exact[:, None, None]), axis=(1, 2))
    bound = 4.0 * EPS * (abs(a) + abs(b) * z_states[0])
    print(f"worst error {float(np.max(err)) / bound:.3f} of the bound")
    assert np.all(err <= bound)


def test_every_slice_is_emitted_once_over_uneven_steps():
    N = 6
    z_slices = np.linspace(9.0, 8.0, 31)                                  # 31 slices: five times round the box
    # uneven steps: one crosses 2 N + 1 slices, one none (it lies between two slices), the rest a few
    z_states = [9.0, 8.99, 8.99 - 13 / 30.0 + 1e-4, 8.55, 8.54, 8.3, 8.0]
    fields = [np.full((N, N, N), float(i)) + np.arange(N)[None, None, :] * 100.0 for i in range(len(z_states))]
    cube, emitted_by = R.build_cone(fields, z_states, z_slices, first_plane=1, axis=2)
    assert cube.shape[0] == 31 and emitted_by == sorted(emitted_by)
    counts = np.bincount(emitted_by, minlength=len(z_states))
    assert counts[0] == 0 and counts.sum() == 31 and counts.max() > 2 * N and 0 in counts[1:]
    # slice m comes from plane (first_plane - m) mod N: the plane's mark (100 k) survives the blend of two states of equal planes
    for m in range(31):
        k = (1 - m) % N
        i = emitted_by[m]
        assert np.all(np.abs(cube[m] - 100.0 * k - (i - 1)) <= 1.0 + 1e-9)
        assert z_states[i] <= z_slices[m] <= z_states[i - 1]


def test_slices_lie_a_fixed_comoving_distance_apart():
    from pyc2ray_amd.lightcone import comoving_interval_mpc, slice_redshifts
    from scipy.integrate import quad
    cosmo = _cosmology()
    dchi = 0.75
    z = slice_redshifts(cosmo, 9.0, 8.9, dchi)
    assert z[0] == 9.0 and np.all(np.diff(z) < 0) and z[-1] >= 8.9 and z.size > 20
    hubble = 299792.458 / 70.0
    gaps = np.array([hubble * quad(lambda s: 1.0 / float(cosmo.efunc(s)), z[m + 1], z[m], epsabs=0.0, epsrel=1e-13)[0] for m in range(z.size - 1)])
    assert np.max(np.abs(gaps / dchi - 1.0)) <= 1e-10
    # ... which the class's own distances confirm as far as a difference of two of them can (9 Gpc against 0.75 Mpc)
    chi = np.array([cosmo.comoving_distance(s) for s in z])
    assert np.allclose(-np.diff(chi), dchi, rtol=1e-5)
    total = comoving_interval_mpc(cosmo, z[-1], z[0])
    assert abs(total / ((z.size - 1) * dchi) - 1.0) <= 1e-10
    # the next one would lie below z_end
    assert comoving_interval_mpc(cosmo, 8.9, z[-1]) < dchi
    for bad in (dict(z_start=8.0, z_end=9.0), dict(dchi_mpc=0.0), dict(dchi_mpc=float("nan")), dict(z_start=-1.0), dict(cosmology=object())):
        kw = {"cosmology": cosmo, "z_start": 9.0, "z_end": 8.9, "dchi_mpc": dchi, **bad}
        with pytest.raises(ValueError, match="slice_redshifts: "):
            slice_redshifts(**kw)
    # down to z = 0 and no further
    near = slice_redshifts(cosmo, 0.001, 0.0, 1.0)
    assert near[-1] >= 0.0 and comoving_interval_mpc(cosmo, 0.0, near[-1]) < 1.0
