"""TEST INFRASTRUCTURE: the numpy statement of the light cone (include/asora_hip.h, asora_lightcone_advance):
the field a slice shows, the blend of two fields' planes, and a plain-Python cone builder over a list of states.  Every operation
is one IEEE double operation in the order the header writes, so the device's slices are compared with these byte for byte."""
import numpy as np

XH, XHI, DENSITY, HI = range(4)


def form(kind, x, n, T, nbar, t_gamma=0.0):
    """g of asora_power_spectrum with scale = 1, per cell."""
    if kind == XH:
        return np.array(x, dtype=np.float64)
    if kind == XHI:
        return 1.0 - x
    if kind == DENSITY:
        return n / nbar
    g = (1.0 * (1.0 - x)) * (n / nbar)
    return g * (1.0 - t_gamma / T) if t_gamma > 0.0 else g


def blend(g_prev, g_now, planes, w_prev, w_now, axis):
    """out[t][a][b] = (w_prev[t] g_prev(cell)) + (w_now[t] g_now(cell)), cell at planes[t] along `axis` and (a, b) on the two other
    axes in ascending order: (n, N, N)."""
    N = g_now.shape[0]
    out = np.empty((len(planes), N, N))
    for t, p in enumerate(planes):
        a = float(w_prev[t]) * np.take(g_prev, int(p), axis=axis)
        b = float(w_now[t]) * np.take(g_now, int(p), axis=axis)
        out[t] = a + b
    return out


def weights(z_prev, z_now, z_slices, scale=None):
    """(w_prev, w_now) of the slices at `z_slices` between two states: linear in z, times scale(z_m)."""
    zs = np.array(z_slices, dtype=np.float64)
    f = (float(z_prev) - zs) / (float(z_prev) - float(z_now))
    s = np.ones_like(zs) if scale is None else np.array([float(scale(z)) for z in zs], dtype=np.float64)
    return (1.0 - f) * s, f * s


def build_cone(fields, redshifts, z_slices, first_plane=0, axis=2, scale=None):
    """The cone of the formed `fields` at the descending `redshifts`, slices at the descending `z_slices`: state i >= 1 emits every
    slice not yet emitted with z_m >= redshifts[i], from plane (first_plane - m) mod N.  Returns (slices (M, N, N), the state index
    that emitted each slice)."""
    N = fields[0].shape[0]
    out, emitted_by, m = [], [], 0
    for i in range(1, len(fields)):
        ms = []
        while m < len(z_slices) and z_slices[m] >= redshifts[i]:
            ms.append(m)
            m += 1
        if ms:
            w_prev, w_now = weights(redshifts[i - 1], redshifts[i], [z_slices[q] for q in ms], scale)
            planes = [(first_plane - q) % N for q in ms]
            out.append(blend(fields[i - 1], fields[i], planes, w_prev, w_now, axis))
            emitted_by += [i] * len(ms)
    cube = np.concatenate(out, axis=0) if out else np.zeros((0, N, N))
    return cube, emitted_by


def fields(N, seed):
    """(x, n, T) of a test mesh: an ionised fraction with exact zeros and ones among it, a log-normal density, temperatures over
    four decades."""
    rng = np.random.default_rng(seed)
    shape = (N, N, N)
    x = rng.random(shape)
    x[rng.random(shape) < 0.1] = 0.0
    x[rng.random(shape) < 0.1] = 1.0
    n = 3.0e-4 * np.exp(rng.standard_normal(shape))
    T = 10.0 ** rng.uniform(1.0, 5.0, shape)
    return x, n, T
