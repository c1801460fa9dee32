"""TEST INFRASTRUCTURE: the numpy statement of the mean-free-path bubble-size specification (include/asora_hip.h, asora_bubble_mfp;
DESIGN.md section 4.2d) -- the hash, the selection of the start cells, the directions, the march and the binning.

``rays(mask, seed, n)`` and ``march(mask, start, dir, l_max, periodic)`` are the two entries; ``distribution`` composes them with
``bin_lengths`` into what the library call returns.  `mask` is a boolean (N, N, N) array, True where a cell is in phase
(``in_phase`` makes it from a field)."""
import numpy as np

ENDED, CAPPED, LEFT_BOX = 0, 1, 2
_K0, _K1, _K2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(seed, c):
    """splitmix64 of the c-th state behind `seed`: uint64 arrays throughout (they wrap around silently)."""
    c = np.atleast_1d(np.asarray(c, dtype=np.uint64))
    z = np.full(c.shape, seed, dtype=np.uint64) + (c + np.uint64(1)) * _K0
    z = (z ^ (z >> np.uint64(30))) * _K1
    z = (z ^ (z >> np.uint64(27))) * _K2
    return z ^ (z >> np.uint64(31))


def u01(h):
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def in_phase(field, threshold, phase):
    """Plain comparisons: a NaN is in neither phase."""
    return field >= threshold if phase == 0 else field < threshold


def mask_words(mask):
    """The device layout of a mask: (words (N, N, W) uint64 with bit k & 63 of word k >> 6, row counts (N, N) uint32)."""
    N = mask.shape[0]
    W = (N + 63) // 64
    padded = np.zeros((N, N, W * 64), dtype=np.uint64)
    padded[:, :, :N] = mask
    words = (padded.reshape(N, N, W, 64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64)
    return words, mask.sum(axis=2).astype(np.uint32)


def rays(mask, seed, n):
    """(start (n, 3) int64, dir (n, 3) float64) of rays 0 ... n - 1; the mask must hold an in-phase cell."""
    cells = np.flatnonzero(mask)
    N = mask.shape[0]
    r4 = np.uint64(4) * np.arange(n, dtype=np.uint64)
    u = mix(seed, r4) % np.uint64(cells.size)
    start = np.stack(np.unravel_index(cells[u.astype(np.int64)], (N, N, N)), axis=1).astype(np.int64)
    mu = 2.0 * u01(mix(seed, r4 + np.uint64(1))) - 1.0
    phi = 2.0 * np.pi * u01(mix(seed, r4 + np.uint64(2)))
    s = np.sqrt(1.0 - mu * mu)
    return start, np.stack([s * np.cos(phi), s * np.sin(phi), mu], axis=1)


def march(mask, start, dir, l_max, periodic):
    """(length (n,) float64, status (n,) int32) of the rays: exact cell traversal from the cell centres, all rays at once."""
    N = mask.shape[0]
    n = start.shape[0]
    d = np.asarray(dir, dtype=np.float64)
    step = np.sign(d).astype(np.int64)
    with np.errstate(divide="ignore"):
        tdelta = np.where(d != 0.0, 1.0 / np.abs(d), np.inf)
    cell = np.array(start, dtype=np.int64)
    m = np.zeros((n, 3))
    length, status = np.zeros(n), np.full(n, -1, dtype=np.int32)
    live = np.arange(n)
    while live.size:
        tmax = (m[live] + 0.5) * tdelta[live]
        axis = np.argmin(tmax, axis=1)                   # (the first of equal minima: the lowest axis)
        t = tmax[np.arange(live.size), axis]
        capped = t > l_max
        length[live[capped]], status[live[capped]] = l_max, CAPPED
        live, axis, t = live[~capped], axis[~capped], t[~capped]
        cell[live, axis] += step[live, axis]
        m[live, axis] += 1.0
        if periodic:
            cell[live] %= N
            left = np.zeros(live.size, dtype=bool)
        else:
            left = np.any((cell[live] < 0) | (cell[live] >= N), axis=1)
        length[live[left]], status[live[left]] = t[left], LEFT_BOX
        live, t = live[~left], t[~left]
        c = cell[live]
        ended = ~mask[c[:, 0], c[:, 1], c[:, 2]]
        length[live[ended]], status[live[ended]] = t[ended], ENDED
        live = live[~ended]
    return length, status


def bin_lengths(edges, length, status):
    """(counts (nb,), tallies (ended, capped, left_box, underflow, overflow), moments (sum L, sum L^2)) of a per-ray record."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    L = length[status == ENDED]
    b = np.searchsorted(edges, L, "right") - 1
    counts = np.bincount(b[(b >= 0) & (b < nb)], minlength=nb).astype(np.uint64)
    tallies = np.array([L.size, np.sum(status == CAPPED), np.sum(status == LEFT_BOX), np.sum(b < 0), np.sum(b >= nb)], dtype=np.uint64)
    return counts, tallies, np.array([np.sum(L), np.sum(L * L)])


def distribution(mask, seed, n, l_max, periodic, edges):
    """What asora_bubble_mfp returns for the mask, all on the CPU: (counts, tallies with n_phase behind them, moments)."""
    n_phase = int(mask.sum())
    nb = len(edges) - 1
    if n == 0 or n_phase == 0:
        return np.zeros(nb, dtype=np.uint64), np.array([0, 0, 0, 0, 0, n_phase], dtype=np.uint64), np.zeros(2)
    start, d = rays(mask, seed, n)
    counts, tallies, moments = bin_lengths(edges, *march(mask, start, d, l_max, periodic))
    return counts, np.append(tallies, np.uint64(n_phase)), moments


def blob_field(N, seed):
    """A uniform-random field in [0, 1) with a seeded smooth blob of high values laid over it: short rays in the noise, long ones in
    the blob."""
    rng = np.random.default_rng(seed)
    x = rng.random((N, N, N))
    centre = rng.uniform(0.3 * N, 0.7 * N, size=3)
    g = np.arange(N)
    r2 = ((g[:, None, None] - centre[0]) ** 2 + (g[None, :, None] - centre[1]) ** 2 + (g[None, None, :] - centre[2]) ** 2)
    return np.maximum(x, 1.2 * np.exp(-r2 / (2.0 * (0.22 * N) ** 2)))
