"""The loudness stage restated in fp64 (numpy): the contract the kernels of csrc/loudness.hip are checked against.

K-weighting and gating as ITU-R BS.1770-4 states them at 48 kHz, the true peak by 4x oversampling (the method of its Annex 2,
with the project's own Kaiser-windowed-sinc taps), the static gain and the look-ahead limiter as DESIGN §16 defines them.  Nothing
here imports the package: the taps and the state matrix are rebuilt from the definitions, so the host tables are checked too."""
import math

import numpy as np

FS, HOP, CHUNK = 48000, 4800, 480
SOS = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]], dtype=np.float64)
U32 = 2.0 ** -24


# ----------------------------------------------------------------------------- K-weighting
def kweight(x):
    """x [..., N] -> the cascade's output in fp64, sequential, zero initial state (scipy's sosfilt: transposed direct form II)."""
    from scipy.signal import sosfilt
    return sosfilt(SOS, np.asarray(x, dtype=np.float64), axis=-1)


def _step(x, st):
    """One sample of the cascade for a vector of independent filters: x [M], st [4, M] (s1, s2, t1, t2), updated in place."""
    (b0, b1, b2, _, a1, a2), (B0, B1, B2, _, A1, A2) = SOS
    y1 = b0 * x + st[0]
    st[0] = b1 * x - a1 * y1 + st[1]
    st[1] = b2 * x - a2 * y1
    y2 = B0 * y1 + st[2]
    st[2] = B1 * y1 - A1 * y2 + st[3]
    st[3] = B2 * y1 - A2 * y2
    return y2


def homogeneous_transition(chunk=CHUNK):
    """[4, 4]: column j = the state after `chunk` zero-input samples from the unit state e_j (the filter itself, not a matrix power)."""
    st = np.eye(4)
    zero = np.zeros(4)
    for _ in range(chunk):
        _step(zero, st)
    return st


def hop_energies(x):
    """x [B, C, N] -> e [B, C, N // 4800] from the sequential filter."""
    x = np.asarray(x, dtype=np.float64)
    nh = x.shape[-1] // HOP
    y = kweight(x)[..., :nh * HOP]
    return (y.reshape(*x.shape[:-1], nh, HOP) ** 2).sum(-1)


def hop_energies_chunked(x, T, chunk=CHUNK):
    """The kernels' restatement: every chunk from zero state, the carry s_{k+1} = T s_k + end_k, every chunk again from its true
    state with sum y^2 accumulated sample by sample, the chunk sums of a hop added in chunk order."""
    x = np.asarray(x, dtype=np.float64)
    lead = x.shape[:-1]
    nh = x.shape[-1] // HOP
    nck = nh * (HOP // chunk)
    xc = x.reshape(-1, x.shape[-1])[:, :nck * chunk].reshape(-1, nck, chunk)          # [rows, nck, chunk]
    rows = xc.shape[0]
    flat = xc.reshape(rows * nck, chunk)
    st = np.zeros((4, rows * nck))
    for i in range(chunk):
        _step(flat[:, i], st)
    ends = st.reshape(4, rows, nck)
    init = np.zeros((4, rows, nck))
    s = np.zeros((4, rows))
    for k in range(nck):
        init[:, :, k] = s
        s = T @ s + ends[:, :, k]
    st = init.reshape(4, rows * nck).copy()
    acc = np.zeros(rows * nck)
    for i in range(chunk):
        y = _step(flat[:, i], st)
        acc = acc + y * y
    acc = acc.reshape(rows, nh, HOP // chunk)
    e = np.zeros((rows, nh))
    for k in range(HOP // chunk):
        e = e + acc[:, :, k]
    return e.reshape(*lead, nh)


# ----------------------------------------------------------------------------- gating
def gate(e):
    """e [C, nh] of ONE clip -> dict(lufs, gamma, block_lufs [nb], z [nb], n_abs, n_rel)."""
    e = np.asarray(e, dtype=np.float64)
    nh = e.shape[-1]
    nb = nh - 3
    if nb < 1:
        return dict(lufs=-math.inf, gamma=-math.inf, block_lufs=np.zeros(0), z=np.zeros(0), n_abs=0, n_rel=0)
    z = np.stack([e[:, j:j + 4].sum() for j in range(nb)]) / 19200.0
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return dict(lufs=-math.inf, gamma=-math.inf, block_lufs=l, z=z, n_abs=0, n_rel=0)
    gamma = -0.691 + 10.0 * math.log10(z[keep].mean()) - 10.0
    keep2 = keep & (l > gamma)
    lufs = -0.691 + 10.0 * math.log10(z[keep2].mean()) if keep2.any() else -math.inf
    return dict(lufs=lufs, gamma=gamma, block_lufs=l, z=z, n_abs=int(keep.sum()), n_rel=int(keep2.sum()))


def integrated_loudness(x):
    """x [C, N] or [N] of one clip at 48 kHz -> LUFS."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return gate(hop_energies(x))["lufs"]


# ----------------------------------------------------------------------------- true peak
def prototype():
    k = np.arange(-24, 25, dtype=np.float64)
    return np.sinc(k / 4.0) * np.kaiser(49, 8.0)


def phase_taps():
    """[4, 12]: row r, column j + 5 = h[r - 4 j] (h zero outside -24 .. 24), each phase scaled to sum to 1."""
    h = prototype()
    out = np.zeros((4, 12))
    for r in range(4):
        for j in range(-5, 7):
            k = r - 4 * j
            out[r, j + 5] = h[k + 24] if -24 <= k <= 24 else 0.0
        out[r] /= out[r].sum()
    return out


def oversampled(x, taps=None):
    """x [N] -> (u [3, N]: u[r - 1, n] = u[4 n + r], a [3, N] = sum_j |x[n + j] h|: the magnitude sum of the same products)."""
    taps = phase_taps() if taps is None else taps
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    xp = np.concatenate([np.zeros(5), x, np.zeros(6)])
    u, a = np.zeros((3, N)), np.zeros((3, N))
    for r in (1, 2, 3):
        for j in range(-5, 7):
            t = xp[5 + j:5 + j + N] * taps[r, j + 5]
            u[r - 1] += t
            a[r - 1] += np.abs(t)
    return u, a


def envelope(x, taps=None):
    """x [C, N] -> (p [N], bound [N]): the peak envelope and the fp32 bound of a device value of it - every |u| is a 12-term
    fp32 FMA chain over fp32-rounded taps (13 * 2^-24 * sum |x h|) and max / abs are exact and 1-Lipschitz; one more rounding
    covers the representation of the result."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    p = np.zeros(x.shape[1])
    bound = np.zeros(x.shape[1])
    for c in range(x.shape[0]):
        u, a = oversampled(x[c], taps)
        p = np.maximum(p, np.maximum(np.abs(x[c]), np.abs(u).max(0)))
        bound = np.maximum(bound, 13 * U32 * a.max(0))
    return p, bound + U32 * p


def true_peak(x):
    return float(envelope(x)[0].max())


# ----------------------------------------------------------------------------- limiter
def limiter_gain(p, G, c, W):
    """p [N] the envelope, G the static gain, c the linear ceiling, W the look-ahead in samples -> (g [N], r [N]):
    r = min(1, c / (G p)) (1 outside [0, N)), gmin[m] = min r[m .. m + W] for m in [-W, N), g[n] = mean gmin[n - W .. n], held at
    r[n] (every window contains n, so the mean is <= r[n] in exact arithmetic: the min only removes its rounding)."""
    r = reduction(p, G, c)
    return gain_curve(r, W), r


def reduction(p, G, c):
    with np.errstate(divide="ignore"):
        return np.minimum(1.0, c / (G * np.asarray(p, dtype=np.float64)))


def gain_curve(r, W):
    """g of r [N] (see limiter_gain); monotone in r: a larger r nowhere gives a smaller g."""
    rp = np.concatenate([np.ones(W), r, np.ones(W)])                       # samples -W .. N + W - 1
    gmin = np.lib.stride_tricks.sliding_window_view(rp, W + 1).min(-1)     # m = -W .. N - 1
    g = np.lib.stride_tricks.sliding_window_view(gmin, W + 1).sum(-1) / (W + 1)
    return np.minimum(g, r)


def untouched(r, W):
    """[N] bool: r == 1 on all of [n - W, n + W] (1 outside the clip) - there g is exactly 1."""
    rp = np.concatenate([np.ones(W), r, np.ones(W)])
    return np.lib.stride_tricks.sliding_window_view(rp, 2 * W + 1).min(-1) == 1.0


def db(v):
    return 20.0 * math.log10(v) if v > 0 else -math.inf
