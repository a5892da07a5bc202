"""The one-wave kernels stop computing the padding of their last 16 x 16 block (csrc/srbdqp_setup1.hpp, PAD / kLastSteps / kLastPivots; csrc/srbdqp_mfma.hpp,
diag16_invert_dpp_packed<NP>): with KS = 60 real variables in 4 x 4 tiles (N = 10, two contacts a step) rows and columns 60 .. 63 of K are zero off the diagonal
and 1.0 on it, and a pass

  runs the last diagonal tile's elimination for its 16 - PAD real pivots, on its real rows alone,
  leaves the k-steps over rows 16 - PAD .. 15 out of P_{NT-1} = W'W,
  leaves them out of every product of I that contracts over block row NT - 1:  Kt[g][NT-1] x Xc[NT-1].

Here F and I restated in NumPy tile by tile, operation by operation in the kernel's order (a tile product is four k-steps of four rank-1 updates each, added to
the accumulator one after the other; the elimination is diag16_pivot_packed's: d, r = 1 / sqrt(d), y = X_k r, nu = -(S_k r), X_i += nu[i] y), in the FULL form
(16 pivots, every k-step: the kernels until this change) and the LIVE form.  NumPy has no fused multiply-add and its 1 / sqrt is not the kernel's rsqrt, so the
figures are not the GPU's; the two forms share every operation they both do, which is what the comparison needs: what the live form leaves out must be
additions of +-0 to sums of real terms.

  K^-1 in rows and columns below KS: equal BIT FOR BIT between the forms (tobytes), on SPD matrices of size 60 padded to 64 (NT = 4, PAD = 4: one k-step) and
  24 padded to 32 (N = 4, two contacts: NT = 2, PAD = 8: two k-steps), one of them with a -0.0 among its real entries;
  a matrix with n_eff = 54 < KS (real zeros beside the padding: a swing step): bit for bit below n_eff, equal as numbers below KS (a kernel masks those);
  a NaN off the diagonal in block row 3 (inside the last diagonal tile, and in tile (1, 3)): the failure flag of the pivots is set, the same, in both forms;
  the live form's padded rows and columns hold nothing that is not finite when the inputs are finite."""
import numpy as np
import pytest

T = 16


def _hi(d):
    return int(np.array(d, dtype=np.float64).view(np.uint64) >> np.uint64(32))


def diag_invert(S, pivots):
    """diag16_invert_dpp_packed<pivots>: S (16 x 16, its upper triangle is read) -> W = L^-1 (rows at or beyond `pivots`: the identity's), worst pivot word"""
    S = np.triu(S) + np.triu(S, 1).T
    R = np.eye(T)
    worst = 0
    with np.errstate(all="ignore"):
        for k in range(pivots):
            d = S[k, k]
            worst = max(worst, (_hi(d) - 1) & 0xFFFFFFFF)
            r = 1.0 / np.sqrt(d)
            ys, yr = S[k] * r, R[k] * r
            nu = S[k] * -r
            for i in range(k + 1, pivots):           # (the full form: pivots = 16, every row below; the live form never touches a padded row)
                S[i] = S[i] + nu[i] * ys
                R[i] = R[i] + nu[i] * yr
            S[k], R[k] = ys, yr
    return R, worst


def kstep(A, B, o, steps=4):
    """o += A' B over the first `steps` k-steps of four rows: the products of the kernel that contract over the ROW index of two C-layout tiles"""
    with np.errstate(all="ignore"):
        for k in range(4 * steps):
            o = o + np.outer(A[k], B[k])
    return o


def kinv(K, NT, pad):
    """F and I of setup1_pass; pad = 0: the full form.  -> (K^-1 as the tiles hold it, ok)"""
    live, pivots = 4 - pad // 4, 16 - 4 * (pad // 4)
    Kt = {(a, b): K[T * a:T * a + T, T * b:T * b + T].copy() for a in range(NT) for b in range(a, NT)}
    zero = np.zeros((T, T))
    ok = True
    for j in range(NT):
        last = j == NT - 1
        w, worst = diag_invert(Kt[j, j], pivots if last else 16)
        ok = ok and worst < 0x7FEFFFFF
        if not last:
            for b in range(j + 1, NT):
                Kt[j, b] = kstep(w.T, Kt[j, b], zero)                      # panel: U_jb = W_jj K_jb
            for a in range(j + 1, NT):
                for b in range(a, NT):
                    Kt[a, b] = kstep(-Kt[j, a], Kt[j, b], Kt[a, b])       # trailing: K_ab -= U_ja' U_jb
            for l in range(j + 1, NT):
                Kt[j, l] = kstep(-Kt[j, l], w, zero)                      # -V_lj = -U_jl' W_jj
        Kt[j, j] = kstep(w, w, zero, live if last else 4)                 # P_j = W_jj' W_jj
    X = {}
    for cb in range(NT - 1, -1, -1):
        Xc = {l: X[cb, l].T.copy() for l in range(cb + 1, NT)}
        for g in range(cb, -1, -1):
            o = Kt[cb, cb] if g == cb else zero
            for l in range(g + 1, NT):
                o = kstep(Kt[g, l], Xc[l], o, live if l == NT - 1 else 4)
            Xc[g] = o
            X[g, cb] = o
    out = np.zeros((T * NT, T * NT))
    for (a, b), v in X.items():
        out[T * a:T * a + T, T * b:T * b + T] = v
        out[T * b:T * b + T, T * a:T * a + T] = v.T
    return out, ok


def _spd(n, size, seed, minus_zero=False):
    """a dense SPD matrix of size n in the corner of the identity of size `size`, as kasm_rows / dcol pad K"""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n + 8, n))
    K = np.eye(size)
    K[:n, :n] = G.T @ G + (40.0 if minus_zero else 0.5) * np.eye(n)      # (the larger shift: zeroing three entries of size sqrt(n) must leave K positive definite)
    if minus_zero:
        for a, b in ((3, n - 2), (n - 5, n - 1), (17, 20)):
            K[a, b] = K[b, a] = -0.0
    return K


SHAPES = {"n10_60_of_64": (60, 4, 4), "n4_24_of_32": (24, 2, 8)}          # KS, NT, PAD


@pytest.mark.parametrize("minus_zero", [False, True], ids=["dense", "minus_zero_entry"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_live_form_gives_the_full_forms_bits_below_ks(shape, minus_zero):
    ks, NT, pad = SHAPES[shape]
    for seed in (1, 2, 3):
        K = _spd(ks, T * NT, 3300 + 10 * ks + seed, minus_zero)
        if minus_zero:
            assert np.signbit(K[3, ks - 2]) and K[3, ks - 2] == 0.0
        full, ok_f = kinv(K, NT, 0)
        live, ok_l = kinv(K, NT, pad)
        assert ok_f and ok_l
        assert full[:ks, :ks].tobytes() == live[:ks, :ks].tobytes()
        assert np.isfinite(live).all()
        ref = np.linalg.inv(K[:ks, :ks])
        assert np.abs(live[:ks, :ks] - ref).max() <= 1e-9 * np.abs(ref).max()      # (and it IS the inverse: a restatement that dropped real terms would agree with itself)
        # what the padded positions hold: zeros between padded and real, the identity in the full form's padded block and 0 in the live form's
        assert not full[:ks, ks:].any() and not live[:ks, ks:].any() and not live[ks:, ks:].any()
        assert np.array_equal(full[ks:, ks:], np.eye(T * NT - ks))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_real_zeros_beside_the_padding(shape):
    """n_eff = KS - 6: a swing step.  Rows n_eff .. KS - 1 are identity rows like the padding, but inside the live k-steps."""
    ks, NT, pad = SHAPES[shape]
    ne = ks - 6
    K = _spd(ne, T * NT, 3400 + ks)
    full, ok_f = kinv(K, NT, 0)
    live, ok_l = kinv(K, NT, pad)
    assert ok_f and ok_l
    assert full[:ne, :ne].tobytes() == live[:ne, :ne].tobytes()
    assert np.array_equal(full[:ks, :ks], live[:ks, :ks])
    assert np.isfinite(live).all()


@pytest.mark.parametrize("where", [(50, 55), (20, 52), (49, 59)], ids=["last_diagonal_tile", "tile_1_3", "last_real_column"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_entry_in_block_row_3_fails_the_same_pivots(where, value):
    ks, NT, pad = SHAPES["n10_60_of_64"]
    K = _spd(ks, T * NT, 3500)
    K[where] = K[where[::-1]] = value
    full, ok_f = kinv(K, NT, 0)
    live, ok_l = kinv(K, NT, pad)
    assert not ok_f and not ok_l


def test_the_padded_pivots_are_exactly_one():
    """what the full elimination computes on rows 12 .. 15 of the last tile: pivots of 1.0 (1 / sqrt(1.0) = 1.0), rows of W equal to the identity's, +0 included"""
    K = _spd(60, 64, 3600)
    S = K[48:, 48:]
    wf, worst_f = diag_invert(S, 16)
    wl, worst_l = diag_invert(S, 12)
    assert wf.tobytes() == wl.tobytes()
    assert wf[12:].tobytes() == np.eye(T)[12:].tobytes()
    assert (worst_f < 0x7FEFFFFF) and (worst_l < 0x7FEFFFFF)
