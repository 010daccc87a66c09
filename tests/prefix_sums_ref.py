"""NumPy model of the box sums of one 64-column window of the fast aggregation kernel (k_match_fast.h: fast_pass_pair),
in the kernel's own float32 operations and operation order, in both forms:

  sliding   Vs += R3[q] - R3[q-21],  Cs += R9[q-6] - R9[q-15],  Hs += R21[q-9] - R21[q-12]
  prefix    P[q] = P[q-1] + R3[q];  PC = P[c-3] + P[c] + P[c+3];  PH = PC[c-6] + PC[c+6] + P[c];
            Vs = P[q] - P[q-21],  Cs = PC[q-6] - PC[q-15],  Hs = PH[q-9] - PH[q-12]

Input: s[TH + 22][64], the per-pixel terms 255 K^2 - |L - R| of the window's tile rows in integer units (exact in float32).
Output: (Vs, Cs, Hs) of every output row o = q - 20 at the 42 valid columns (lanes 11 .. 52), float32 [3][TH][42].
Columns outside the window read as zero, like the slack entries of the exchange row -- they only reach halo lanes."""
import numpy as np

HALO, VALID = 11, 42
F = np.float32


def _shift(a, k):
    """a[:, c + k] with zeros shifted in."""
    out = np.zeros_like(a)
    if k > 0:
        out[:, :-k] = a[:, k:]
    elif k < 0:
        out[:, -k:] = a[:, :k]
    else:
        out[:] = a
    return out


def r3_rows(s):
    """R3[q], q = 0 .. TH + 19: the 3 x 3 cost summed over 3 columns (integers far below 2^24: exact in any order)."""
    s = np.asarray(s, dtype=F)
    v3 = (s[:-2] + s[1:-1]) + s[2:]
    cv = (_shift(v3, -1) + v3) + _shift(v3, 1)
    return ((_shift(cv, -1) + cv) + _shift(cv, 1)).astype(F)


def _r9(x):
    return ((_shift(x, -3) + x) + _shift(x, 3)).astype(F)


def _r21(x9, x3):
    return ((_shift(x9, -6) + _shift(x9, 6)) + x3).astype(F)


def sliding(s):
    r3 = r3_rows(s)
    nq, th = r3.shape[0], r3.shape[0] - 20
    r9, r21 = _r9(r3), _r21(_r9(r3), r3)
    vs, cs, hs = (np.zeros(64, F) for _ in range(3))
    out = np.zeros((3, th, 64), F)
    for q in range(nq):
        vs = vs + r3[q]
        if q >= 21:
            vs = vs - r3[q - 21]
        if q >= 12:
            cs = cs + r9[q - 6]
        if q >= 21:
            cs = cs - r9[q - 15]
        if q >= 18:
            hs = hs + r21[q - 9]
        if q >= 21:
            hs = hs - r21[q - 12]
        if q >= 20:
            out[:, q - 20] = vs, cs, hs
    return out[:, :, HALO:HALO + VALID]


def prefix(s):
    r3 = r3_rows(s)
    nq, th = r3.shape[0], r3.shape[0] - 20
    p = np.zeros_like(r3)
    p[0] = r3[0]
    for q in range(1, nq):
        p[q] = p[q - 1] + r3[q]
    pc = _r9(p)
    ph = _r21(pc, p)
    out = np.zeros((3, th, 64), F)
    for q in range(20, nq):
        vs = p[q] - p[q - 21] if q >= 21 else p[q]
        out[:, q - 20] = vs, pc[q - 6] - pc[q - 15], ph[q - 9] - ph[q - 12]
    return out[:, :, HALO:HALO + VALID], float(ph[:th + 11].max())      # ... and the largest prefix a box reads (tile row th + 10)


def exact_in_float64(s):
    """The same box sums in float64 integers: what both forms must give when nothing rounds."""
    s = np.asarray(s, dtype=np.float64)
    v3 = s[:-2] + s[1:-1] + s[2:]
    cv = _shift(v3, -1) + v3 + _shift(v3, 1)
    r3 = _shift(cv, -1) + cv + _shift(cv, 1)
    r9 = _shift(r3, -3) + r3 + _shift(r3, 3)
    r21 = _shift(r9, -6) + _shift(r9, 6) + r3
    th = r3.shape[0] - 20
    out = np.zeros((3, th, 64))
    for o in range(th):
        q = o + 20
        out[0, o] = r3[q - 20:q + 1].sum(0)
        out[1, o] = r9[q - 14:q - 5].sum(0)
        out[2, o] = r21[q - 11:q - 8].sum(0)
    return out[:, :, HALO:HALO + VALID]
