"""CPU: the certificate of the column kernel's even/odd long pass (csrc/gauss_col_kernel.inc, csrc/ia3_col_weights.h).

The kernel forms E[q] = v[q] + v[Z-1-q] and O[q] = v[q] - v[Z-1-q] once per column and computes a mirror pair of outputs
as a = P + M, b = P - M with P = sum Wp E, M = sum Wm O.  This file restates that arithmetic in NumPy (float64, same order,
weights from the library's own builder) and checks the two statements the kernel's header makes:

(a) |eo - exact| <= C u P with C = 2n + 2 tw + 6, P = (a + b) / 2 — against the exact sum (math.fsum over error-free
    products).  NumPy has no fused multiply-add, so every term of the restated chains carries two roundings where the
    kernel's carries one; the kernel's (tighter) bound is asserted on it all the same.
(b) every output whose float32 rounding / uint16 truncation differs between the even/odd sum and NI_Correlate1D's own
    sequence is caught by "lopsided pair, or within the guard of a quantisation boundary", with the library's constants.
"""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "imageanalysis3_amd", "csrc")
U = 2.0 ** -53
R = 30
NCOL = 200000
CHUNK = 4000
MODES = {"reflect": 0, "nearest": 1}


def _lib():
    from imageanalysis3_amd import _lib as L
    return L, L.lib()


def _taps():
    L, _ = _lib()
    w, r = L.gaussian_taps(7.5, 4.0)
    assert r == R
    return np.ascontiguousarray(np.asarray(w, np.float64)[r:])   # w[0 .. R], symmetric kernel


def _lopsided_k():
    with open(os.path.join(CSRC, "ia3_col_weights.h")) as f:
        k = int(re.search(r"constexpr int COL_LOPSIDED_K = (\d+);", f.read()).group(1))
    with open(os.path.join(CSRC, "gauss_col_kernel.inc")) as f:
        assert int(re.search(r"constexpr int COL_K = (\d+);", f.read()).group(1)) == k
    return k


def _border(q, n, mode):
    if mode == "nearest":
        return min(max(q, 0), n - 1)
    q %= 2 * n
    return q if q < n else 2 * n - 1 - q


def _weights(Z, mode, w):
    """W, Wp, Wm as csrc/ia3_col_weights.h builds them (float64, taps added in the order -R .. R), and the stream."""
    H, rows = Z // 2, (Z + 1) // 2
    W = np.zeros((rows, Z))
    for z in range(rows):
        for p in range(Z):
            acc = 0.0
            for j in range(-R, R + 1):
                if _border(z + j, Z, mode) == p:
                    acc += float(w[abs(j)])
            W[z, p] = acc
    Wp = (W[:, :H] + W[:, ::-1][:, :H]) * 0.5
    Wm = (W[:, :H] - W[:, ::-1][:, :H]) * 0.5
    stream = []
    for z in range(rows):
        for q in range(H):
            stream.append(Wp[z, q])
            if z < H:
                stream.append(Wm[z, q])
        if Z & 1:
            stream.append(W[z, H])
    return W, Wp, Wm, np.array(stream)


def _tw(Z, mode):
    return R if mode == "nearest" else 2 * ((2 * R + 1 + 2 * Z - 1) // (2 * Z)) - 1


def _evenodd(cols, Z, W, Wp, Wm):
    """The kernel's long pass on cols (Z, n) float64 (one column per column): outputs (Z, n), and P, |M| per output."""
    H, odd = Z // 2, Z & 1
    E = cols[:H] + cols[::-1][:H]
    O = cols[:H] - cols[::-1][:H]
    P = Wp[:, 0, None] * E[0][None, :]
    M = Wm[:H, 0, None] * O[0][None, :]
    for q in range(1, H):
        P = P + Wp[:, q, None] * E[q][None, :]
        M = M + Wm[:H, q, None] * O[q][None, :]
    if odd:
        P = P + W[:, H, None] * cols[H][None, :]
    out, Pz, Mz = np.empty_like(cols), np.empty_like(cols), np.zeros_like(cols)
    out[:H] = P[:H] + M
    out[::-1][:H] = P[:H] - M
    Pz[:H] = P[:H]
    Pz[::-1][:H] = P[:H]
    Mz[:H] = np.abs(M)
    Mz[::-1][:H] = np.abs(M)
    if odd:
        out[H] = P[H]
        Pz[H] = P[H]
    return out, Pz, Mz


def _reference(cols, Z, mode, w):
    """NI_Correlate1D's sequence on cols (Z, n): acc = v[z] w0; for j = R .. 1: acc = acc + (v[z-j] + v[z+j]) w[j]."""
    idx = np.array([[_border(z + j, Z, mode) for z in range(Z)] for j in range(-R, R + 1)])
    acc = cols * w[0]
    for j in range(R, 0, -1):
        acc = acc + (cols[idx[R - j]] + cols[idx[R + j]]) * w[j]
    return acc


def _uncertain(s, guard, f32):
    """ia3_gauss_dev.h: uncertain<float> / uncertain<uint16_t>."""
    if f32:
        bits = s.view(np.uint64)
        lo, hi = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32), (bits >> np.uint64(32)).astype(np.uint32)
        c = np.uint32(min(guard, 0x10000000))
        near_mid = ((lo & np.uint32(0x1FFFFFFF)) - (np.uint32(0x10000000) - c)) <= np.uint32(2) * c
        odd_exp = ((hi - np.uint32(0x39B00000)) >= np.uint32(0x7FF00000 - 0x39B00000)) & ((hi | lo) != 0)
        return near_mid | odd_exp
    return (s != 0.0) & (np.abs(s - np.rint(s)) <= s * (float(guard) * 2.220446049250313e-16))


def _quantise(s, f32):
    return s.astype(np.float32) if f32 else s.astype(np.int64)   # round to nearest even / truncation of a non-negative sum


def _columns(kind, Z, rng, n):
    if kind == "background_noise_f32":
        return (400.0 + rng.gamma(2.0, 60.0, size=(n, Z))).astype(np.float32), True
    if kind == "poisson_u16":
        return rng.poisson(rng.uniform(1.0, 3000.0, size=(n, 1)), size=(n, Z)).astype(np.uint16), False
    if kind in ("half_zero_f32", "half_zero_mirror_f32"):
        c = np.zeros((n, Z), np.float32)
        c[:, Z // 2 + 3:] = rng.uniform(0.0, 6e4, size=(n, Z - Z // 2 - 3)).astype(np.float32)
        return (c if kind == "half_zero_f32" else c[:, ::-1].copy()), True
    if kind == "blocks_u16":   # piecewise constant: every sum is within a few ulps of an integer, truncation flips on the last bit
        c = np.repeat(rng.randint(1, 65535, size=(n, 1)), Z, axis=1)
        step = rng.randint(0, Z + 1, size=(n, 1))
        c = np.where(np.arange(Z)[None, :] >= step, c // 3, c)
        return c.astype(np.uint16), False
    raise ValueError(kind)


KINDS = ("background_noise_f32", "poisson_u16", "half_zero_f32", "half_zero_mirror_f32", "blocks_u16")


def test_weight_stream_and_guard_are_the_library_s():
    """The restated W / Wp / Wm stream equals ia3_col_weights bit for bit, and the default guard is the derived one."""
    L, lib = _lib()
    w = _taps()
    K = _lopsided_k()
    for Z in (16, 25, 33, 50, 60, 64):
        for mode, code in MODES.items():
            stream = _weights(Z, mode, w)[3]
            n = lib.ia3_col_weights(Z, R, code, L.ptr(w), None, 0)
            assert n == (len(stream) + 15) // 16 * 16 and len(stream) == (Z // 2) * Z + (Z & 1) * ((Z + 1) // 2)
            got = np.full(n, np.nan)
            assert lib.ia3_col_weights(Z, R, code, L.ptr(w), L.ptr(got), n) == n
            assert np.array_equal(got[:len(stream)].view(np.uint64), stream.view(np.uint64)), (Z, mode)
            assert not got[len(stream):].any()
            nterms = (Z + 1) // 2
            assert lib.ia3_col_guard(Z, R, code) == K * (2 * nterms + 2 * _tw(Z, mode) + 6) + 3 * R + 4
    assert lib.ia3_col_guard(50, R, 0) == 326


def test_weights_keep_the_symmetry_the_bound_uses():
    """|Wm| <= Wp as computed (the M chain is bounded term by term by the P chain), and no W entry sums more than tw + 1 taps."""
    w = _taps()
    for Z in (16, 25, 33, 50, 60, 64):
        for mode in MODES:
            W, Wp, Wm, _ = _weights(Z, mode, w)
            assert (np.abs(Wm) <= Wp).all() and (W >= 0).all()
            hits = np.zeros((Z, Z), int)
            for z in range(Z):
                for j in range(-R, R + 1):
                    hits[z, _border(z + j, Z, mode)] += 1
            assert hits.max() <= _tw(Z, mode) + 1, (Z, mode, hits.max())
            assert np.array_equal(hits[::-1, ::-1], hits)   # W[Z-1-z][Z-1-p] = W[z][p]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("Z", (25, 33, 50, 60))
@pytest.mark.parametrize("kind", KINDS)
def test_evenodd_sum_within_bound_and_mismatches_caught(kind, Z, mode):
    _, lib = _lib()
    w = _taps()
    K = _lopsided_k()
    guard = lib.ia3_col_guard(Z, R, MODES[mode])
    W, Wp, Wm, _ = _weights(Z, mode, w)
    Cb = 2 * ((Z + 1) // 2) + 2 * _tw(Z, mode) + 6
    rng = np.random.RandomState(1000 * Z + 10 * KINDS.index(kind) + MODES[mode])
    # Veltkamp split of the taps: hi has 26 bits, lo the rest, so that hi * x and lo * x are exact for float32 / uint16 x
    t = w * (2.0 ** 27 + 1.0)
    w_hi = t - (t - w)
    w_lo = w - w_hi
    mismatches = caught_total = 0
    worst = 0.0
    for start in range(0, NCOL, CHUNK):
        raw, f32 = _columns(kind, Z, rng, CHUNK)
        cols = np.ascontiguousarray(raw.T.astype(np.float64))   # (Z, n)
        eo, P, absM = _evenodd(cols, Z, W, Wp, Wm)
        ref = _reference(cols, Z, mode, w)
        differ = _quantise(eo, f32) != _quantise(ref, f32)
        caught = (absM > P * (1.0 - 1.0 / K)) | _uncertain(eo, guard, f32)
        assert not (differ & ~caught).any(), (kind, Z, mode, int((differ & ~caught).sum()))
        mismatches += int(differ.sum())
        caught_total += int(caught.sum())
        if start == 0:   # (a): the first columns of the case against the exact sum
            for c in range(48):
                ex = []
                for z in range(Z):
                    xs = [float(cols[_border(z + j, Z, mode), c]) for j in range(-R, R + 1)]
                    terms = [x * float(w_hi[abs(j)]) for x, j in zip(xs, range(-R, R + 1))] + \
                            [x * float(w_lo[abs(j)]) for x, j in zip(xs, range(-R, R + 1))]
                    ex.append((math.fsum(terms), terms))
                for z in range(Z):
                    Pex = 0.5 * (ex[z][0] + ex[Z - 1 - z][0])
                    err = abs(math.fsum(ex[z][1] + [-float(eo[z, c])]))   # exact difference, rounded once
                    assert err <= Cb * U * Pex, (kind, Z, mode, c, z, err / (U * Pex) if Pex else err)
                    if Pex:
                        worst = max(worst, err / (U * Pex))
    print("%s Z=%d %s: guard %d, bound %d u P (worst seen %.1f), %d of %d outputs quantise differently, %d take the reference tail"
          % (kind, Z, mode, guard, Cb, worst, mismatches, NCOL * Z, caught_total))
    if kind in ("background_noise_f32", "poisson_u16"):   # the tail stays an exception on ordinary data
        assert caught_total <= 1e-4 * NCOL * Z
