"""The first panel tile of a block row rides the packed tile inversion (csrc/srbdqp_mfma.hpp, diag16_invert_dpp_packed<16, true>; csrc/srbdqp_setup1.hpp, F):
register X_i holds row i of S on DPP rows 0 and 2, row i of R (the identity at the start) on row 1 and row i of B = K_{j,j+1} on row 3, where a second copy of R
sat that nobody read.  The pivots do to row 3 what they do to every row -- y = X_k r, X_i += nu[i] y -- which on B is forward substitution: U = L^-1 B comes
out of the elimination and the four matrix-core instructions of W_jj K_{j,j+1} go.

Here the elimination restated in NumPy pivot by pivot on [S | I | B] in the order of diag16_pivot_packed (d, r = 1 / sqrt(d), y = X_k r, nu = S_k (-r),
X_i += nu[i] y for the rows below; NumPy has no fused multiply-add and its 1 / sqrt is not the kernel's rsqrt, so the figures are not the GPU's):

  W is the routine's without B bit for bit, and so is the worst pivot word, whatever B holds -- a NaN or an infinity in B included: B cannot reach `worst`,
  which is formed from S's diagonal alone; it ends in U, and the trailing update carries it to a pivot of a LATER tile, which fails as it did when the panel was a
  product with W (the whole factorisation below);
  U equals forward substitution with the elimination's own L, row by row with the sums in a row of their own (left-looking), to 4 ulps of its largest entry;
  a NaN or an infinity in S fails the same pivots with and without B.

Then K^-1 by the kernel's recurrence with the riding panels (U_{j,j+1} by substitution, the tiles further right by the product with W_jj, P_j, V and the
recurrence of I as tests/test_kinv_recurrence_cpu.py restates them) on that file's six cases at its five rho scales, NT = 2, 3 and 4, n_eff < 16 NT included,
against its np.longdouble inverse and next to its panel scheme: forward substitution is at least as accurate as the product with an explicit inverse, so the
riding form may not lose against the scheme every earlier form was held to --

  per case   worst relative error <= 1.5 x the panel scheme's worst on the same matrices     (0.34 .. 1.40 here; 1.02 with LAPACK's diagonal inverses)
  per matrix                     <= 3 x the panel scheme's on that matrix                    (2.09 at most here; 1.86)
  rows and columns at or beyond n_eff: exactly the identity's / zero.

1.5 and 3 are the slack of the constant between two kappa eps methods (the file above allows the recurrence 2 on one matrix), not figures tuned to pass."""
import numpy as np
import pytest

import test_kinv_recurrence_cpu as kc

T = 16
GOOD = 0x7FEFFFFF


def _hi(d):
    return int(np.array(d, dtype=np.float64).view(np.uint64) >> np.uint64(32))


def ride_invert(S, B=None):
    """diag16_invert_dpp_packed<16, RIDE = B is given>: -> W = L^-1, U = L^-1 B (or None), worst pivot word, L"""
    S = np.triu(S) + np.triu(S, 1).T
    X = np.concatenate([S, np.eye(T)] + ([np.array(B, dtype=np.float64)] if B is not None else []), axis=1)      # [S | I | B]: DPP rows 0 / 2, 1, 3
    L = np.zeros((T, T))
    worst = 0
    with np.errstate(all="ignore"):
        for k in range(T):
            sk = X[k, :T].copy()                     # pk_even_rows: row k of S in every DPP row
            d = sk[k]
            worst = max(worst, (_hi(d) - 1) & 0xFFFFFFFF)
            r = 1.0 / np.sqrt(d)
            y = X[k] * r                             # u | W_k | U_k
            nu = sk * -r
            L[k, k] = r                              # (1 / L[k][k]: what the substitution multiplies by)
            for i in range(k + 1, T):
                L[i, k] = -nu[i]
                X[i] = X[i] + nu[i] * y
            X[k] = y
    return X[:, T:2 * T], (X[:, 2 * T:] if B is not None else None), worst, L


def forward_substitution(L, B):
    """U = L^-1 B row by row, L's diagonal held as its reciprocal: U_k = (B_k - sum_{m<k} L[k][m] U_m) (1 / L[k][k])"""
    U = np.zeros((T, B.shape[1]))
    with np.errstate(all="ignore"):
        for k in range(T):
            acc = B[k].copy()
            for m in range(k):
                acc = acc + -L[k, m] * U[m]
            U[k] = acc * L[k, k]
    return U


def _tile(seed, shift=0.5):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(T + 8, T))
    return G.T @ G + shift * np.eye(T), rng.normal(size=(T, T)) * 3.0


@pytest.mark.parametrize("seed", [3501, 3502, 3503])
def test_w_is_the_routines_without_b_and_u_is_forward_substitution(seed):
    S, B = _tile(seed)
    w0, none, worst0, L0 = ride_invert(S)
    w, U, worst, L = ride_invert(S, B)
    assert none is None
    assert w.tobytes() == w0.tobytes() and worst == worst0 and worst < GOOD
    assert not np.triu(w, 1).any()                                          # exact zeros above the diagonal, as the A operand needs them
    ref = forward_substitution(L, B)
    ulp = np.spacing(np.abs(U).max())
    print("seed", seed, "max |U - substitution|", np.abs(U - ref).max() / ulp, "ulps of the largest entry")
    assert np.abs(U - ref).max() <= 4 * ulp
    Lm = L.copy()
    Lm[np.diag_indices(T)] = 1.0 / np.diag(L)
    assert np.abs(Lm @ U - B).max() <= 64 * np.finfo(float).eps * (np.abs(Lm) @ np.abs(U)).max()      # (and it IS L^-1 B: a restatement can agree with itself)
    assert np.abs(w @ B - U).max() <= 1e-10 * np.abs(U).max()                # what the panel product formed


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "minus_inf"])
def test_b_cannot_reach_the_pivot_word(value):
    S, B = _tile(3510)
    w0, _, worst0, _ = ride_invert(S)
    B[5, 9] = value
    w, U, worst, _ = ride_invert(S, B)
    assert worst == worst0 and worst < GOOD and w.tobytes() == w0.tobytes()
    assert np.isfinite(U[:5]).all() and np.isfinite(np.delete(U, 9, axis=1)).all() and not np.isfinite(U[5:, 9]).all()      # its own column, from its row down


@pytest.mark.parametrize("where", [(0, 0), (3, 7), (7, 7), (15, 15)], ids=["first_pivot", "off_diagonal", "a_pivot", "last_pivot"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_entry_in_s_fails_the_same_pivots(where, value):
    S, B = _tile(3520)
    S[where] = S[where[::-1]] = value
    _, _, worst0, _ = ride_invert(S)
    _, _, worst, _ = ride_invert(S, B)
    assert worst == worst0 and worst >= GOOD


def kinv_ride(K, NT, ride=True):
    """F and I of setup1_pass as matrices (test_kinv_recurrence_cpu's fall-back form) with the elimination above for the diagonal tiles: ride = True takes
    U_{j,j+1} out of it, ride = False forms every panel as W_jj K_jb.  -> K^-1, ok"""
    Kt = kc._blocks(K, NT)
    P, Ut = {}, {}
    ok = True
    with np.errstate(all="ignore"):
        for j in range(NT):
            riding = ride and j + 1 < NT
            Wjj, Uj, worst, _ = ride_invert(Kt[j, j], Kt[j, j + 1] if riding else None)
            ok = ok and worst < GOOD
            P[j] = Wjj.T @ Wjj
            U = {b: (Uj if riding and b == j + 1 else Wjj @ Kt[j, b]) for b in range(j + 1, NT)}
            for b in range(j + 1, NT):
                Ut[j, b] = (U[b].T @ Wjj).T
            for a in range(j + 1, NT):
                for b in range(a, NT):
                    Kt[a, b] = Kt[a, b] - U[a].T @ U[b]
        X = {}
        for cb in range(NT - 1, -1, -1):
            col = {l: X[cb, l].T for l in range(cb + 1, NT)}
            for g in range(cb, -1, -1):
                o = P[cb].copy() if g == cb else np.zeros((T, T))
                for l in range(g + 1, NT):
                    o = o - Ut[g, l] @ col[l]
                col[g] = o
                X[g, cb] = o
    return kc._assemble(X, NT), ok


@pytest.mark.parametrize("case", list(kc.CASES))
def test_kinv_with_riding_panels_is_as_accurate_as_the_panel_scheme(case):
    worst = dict(panel=0.0, ride=0.0, product=0.0, ratio=0.0, moved=0.0)
    nts = set()
    for b, scale, ne, NT, K in kc._matrices(case):
        nts.add(NT)
        ref = kc._inv_longdouble(K[:ne, :ne])
        top = float(np.abs(ref).max())
        Xr, ok_r = kinv_ride(K, NT)
        Xp, ok_p = kinv_ride(K, NT, ride=False)
        assert ok_r and ok_p
        err = {}
        for name, X in (("panel", kc.kinv_panel(K, NT)), ("ride", Xr), ("product", Xp)):
            err[name] = float(np.abs(X[:ne, :ne].astype(np.longdouble) - ref).max()) / top
        pad = Xr.copy()
        pad[:ne, :ne] = 0.0
        assert np.array_equal(pad[ne:, ne:], np.eye(T * NT - ne)) and not pad[:ne, ne:].any() and not pad[ne:, :ne].any(), (case, b, scale, "padding")
        moved = float(np.abs(Xr[:ne, :ne] - Xp[:ne, :ne]).max()) / top
        print(f"{case} QP {b} rho x {scale:g} n_eff {ne} NT {NT}  panel scheme {err['panel']:.2e}  riding {err['ride']:.2e}  every panel a product {err['product']:.2e}"
              f"  K^-1 moved by {moved:.2e}")
        for k in ("panel", "ride", "product"):
            worst[k] = max(worst[k], err[k])
        worst["ratio"] = max(worst["ratio"], err["ride"] / err["panel"])
        worst["moved"] = max(worst["moved"], moved)
        assert err["ride"] <= 3.0 * err["panel"], (case, b, scale, err)
    print(f"{case}: worst relative error of K^-1: panel scheme {worst['panel']:.2e}, riding {worst['ride']:.2e} (x {worst['ride'] / worst['panel']:.2f}; worst on one "
          f"matrix x {worst['ratio']:.2f}), every panel a product {worst['product']:.2e}; riding against product: K^-1 moved by at most {worst['moved']:.2e}")
    assert worst["ride"] <= 1.5 * worst["panel"], worst
    assert nts <= {2, 3, 4}


def test_the_cases_cover_two_three_and_four_tiles():
    assert {(3 * kc.CASES[c][1] * kc.CASES[c][0] + T - 1) // T for c in kc.CASES} == {2, 3, 4}


@pytest.mark.parametrize("where", [(5, 20), (20, 40), (37, 59)], ids=["tile_0_1", "tile_1_2", "tile_2_3"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_entry_in_a_riding_tile_fails_the_factorisation_as_before(where, value):
    """the entry sits in the tile that rides: its own inversion passes, the trailing update puts it on the diagonal tile below, whose pivot fails -- in both forms"""
    for _, scale, ne, NT, K in kc._matrices("n10_s2_single"):
        break
    K = K.copy()
    K[where] = K[where[::-1]] = value
    _, ok_r = kinv_ride(K, NT)
    _, ok_p = kinv_ride(K, NT, ride=False)
    assert not ok_r and not ok_p
    if where[0] < T:                                 # (block row 0 is inverted as it stands: the tile that carries the entry passes)
        _, U, worst, _ = ride_invert(K[:T, :T], K[:T, T:2 * T])
        assert worst < GOOD and not np.isfinite(U).all()
