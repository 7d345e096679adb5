"""The specification of include/tdk_hip_filmic.h restated in NumPy float32: every line is one rounded operation of the header, in
its order.  tests/test_filmic_spec.py holds it to literal per-pixel loops and to its purpose; tests/test_gpu_filmic.py asks the
kernel for its bits."""

import numpy as np

F = np.float32
EV_MIN, EV_MAX, STEPS, TABLE = -20, 12, 32, 1025
ENC_EV_MIN, ENC_TABLE = -16, 513
MAX, LUMA, POWER, NONE = 0, 1, 2, 3
NORMS = {'max': MAX, 'luma': LUMA, 'power': POWER, 'none': NONE}
XMIN = F(2.0 ** -20)
XMAX = np.nextafter(F(4096.0), F(0.0))
BELOW_ONE = np.nextafter(F(1.0), F(0.0))
ENC_LO = F(2.0 ** -16)
REC709 = (0.2126, 0.7152, 0.0722)


def nodes(ev_min=EV_MIN, entries=TABLE):
    """The float64 positions of the nodes (all of them are float32 values)."""
    j = np.arange(entries)
    return (1.0 + (j % STEPS) / STEPS) * 2.0 ** (j // STEPS + ev_min)


def pos(v):
    """v > 0 ? v : +0: a NaN and -0 become +0."""
    with np.errstate(invalid='ignore'):
        return np.where(v > 0, v, F(0.0)).astype(F)


def index(clamped, ev_min):
    """(i, f) of values clamped into the table whose first octave is 2^ev_min."""
    bits = np.ascontiguousarray(clamped, dtype=F).view(np.uint32)
    ex = (bits >> 23).astype(np.int64) - 127
    M = bits & np.uint32(0x7FFFFF)
    i = (ex - ev_min) * STEPS + (M >> 18).astype(np.int64)
    f = (M & np.uint32(0x3FFFF)).astype(F) / F(262144.0)
    return i, f


def lerp(table, i, f):
    return table[i] + f * (table[i + 1] - table[i])


def encode(o, G):
    oc = np.fmin(pos(o), BELOW_ONE)
    i, f = index(np.fmax(oc, ENC_LO), ENC_EV_MIN)
    return np.where(oc < ENC_LO, (oc * F(65536.0)) * G[0], lerp(G, i, f)).astype(F)


def store(v, dtype):
    if dtype == np.uint8:
        return np.rint(np.fmin(np.fmax(v, F(0.0)), F(1.0)) * F(255.0)).astype(np.uint8)
    with np.errstate(over='ignore'):
        return v.astype(dtype)


def filmic(x, curve, G, exposure, norm, weights=REC709, out_dtype=np.float32, return_fires=False):
    """x: (..., 3) float32 or float16; curve: (2, TABLE) float32 (T, D); G: (ENC_TABLE,) float32 or None; exposure: a float32.
    The result has x's shape and out_dtype; with return_fires also the mask of the pixels on which step 5 fired."""
    assert x.shape[-1] == 3 and x.dtype in (np.float32, np.float16)
    T, D = np.asarray(curve, dtype=F).reshape(2, TABLE)
    w = [F(v) for v in weights]
    shape = x.shape
    with np.errstate(all='ignore'):
        x = x.reshape(-1, 3).astype(F)
        p = np.fmin(pos(x * F(exposure)), XMAX)
        p0, p1, p2 = p[..., 0], p[..., 1], p[..., 2]
        if norm == NONE:
            i, f = index(np.fmin(np.fmax(p, XMIN), XMAX), EV_MIN)
            o = lerp(T, i, f)
            fires = np.zeros(len(p), dtype=bool)
        else:
            if norm == MAX:
                N = np.fmax(np.fmax(p0, p1), p2)
            elif norm == LUMA:
                N = (w[0] * p0 + w[1] * p1) + w[2] * p2
            else:
                q0, q1, q2 = p0 * p0, p1 * p1, p2 * p2
                k0, k1, k2 = q0 * p0, q1 * p1, q2 * p2
                den, num = (q0 + q1) + q2, (k0 + k1) + k2
                N = np.where(den > 0, num / np.where(den > 0, den, F(1.0)), F(0.0)).astype(F)
            Nc = np.fmin(np.fmax(N, XMIN), XMAX)
            i, f = index(Nc, EV_MIN)
            y, d = lerp(T, i, f), lerp(D, i, f)
            y3, d3 = y[..., None], d[..., None]
            o = y3 * (F(1.0) + d3 * (p / Nc[..., None] - F(1.0)))
            m = np.fmax(np.fmax(o[..., 0], o[..., 1]), o[..., 2])
            fires = m > 1
            g = (F(1.0) - y) / np.where(fires, m - y, F(1.0))
            pulled = np.where((y >= 1)[..., None], F(1.0), y3 + (o - y3) * g[..., None])
            o = np.where(fires[..., None], pulled, o).astype(F)
        v = o if G is None else encode(o, np.asarray(G, dtype=F))
        out = store(v.astype(F), out_dtype).reshape(shape)
        return (out, fires.reshape(shape[:-1])) if return_fires else out


# ---- inputs the tests share
def specials():
    """Samples at the ends of the domain and on and next to table nodes, each as the first, second and third channel of a coloured
    pixel and as a grey one."""
    f = F
    pick = nodes().astype(f)[[0, 1, 31, 32, 33, 500, 639, 640, 641, 1023, 1024]]
    enc = nodes(ENC_EV_MIN, ENC_TABLE).astype(f)[[0, 1, 32, 511, 512]]
    values = [f(-1.0), f(-0.0), f(0.0), f(np.nan), f(np.inf), f(-np.inf), f(65504.0), f(1.0), f(0.18), XMIN, XMAX, f(4096.0), f(3.0e38), f(2.0 ** -22)]
    for v in (*pick, *enc, XMIN, XMAX, f(1.0)):
        values += [v, np.nextafter(v, f(0.0)), np.nextafter(v, f(np.inf))]
    rows = []
    for v in values:
        rows += [(v, 0.5, 0.25), (0.3, v, 0.1), (0.2, 0.7, v), (v, v, v)]
    return np.array(rows, dtype=f)


def samples(n, dtype, seed=0):
    """(n, 3) of `dtype`: the specials, then colours at every exposure from below the tables to above them, many of them saturated
    (the gamut step fires on those under 'luma' and 'power').  No value is a float32 denormal or has a denormal square or cube."""
    rng = np.random.default_rng(seed)
    s = specials()
    m = max(n - len(s), 0)
    level = np.exp2(rng.uniform(-21.0, 12.5, (m, 1)))
    chroma = np.where(rng.random((m, 3)) < 0.3, rng.uniform(0.0, 0.02, (m, 3)), rng.uniform(0.02, 1.0, (m, 3)))
    chroma[rng.random((m, 3)) < 0.03] = 0.0
    x = (level * chroma).astype(np.float32)
    x[(x != 0) & (np.abs(x) < 2.0 ** -22)] = 0.0
    with np.errstate(over='ignore'):
        return np.concatenate((s, x))[:n].astype(dtype)
