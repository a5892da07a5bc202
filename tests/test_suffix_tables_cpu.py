"""CPU restatement of the one-wave kernel's step tables T1(m), T2(m) (csrc/srbdqp_setup1.hpp, "closed-form tables").

C_k = sum_{l<=k} Rz(yaw_l)' has two non-constant entries, so the kernel forms T1 and T2 from six per-step sums over the
wave-uniform prefix sums (differences-first: every term from C_i - C_m).  These tests check
  * that the six-sum form equals the generic 3 x 3 differences-first form it replaced, and
  * what the suffix-sum form S(m) - (N - m) C_m, Q(m) - C_m'W S(m) - S(m)'W C_m + (N - m) C_m'W C_m would cost in precision:
    T1 a few ulps, T2 up to ~250 ulps at N = 10 (two to three digits, near the end of the horizon).  That still holds 1e-11,
    but on one wave the differences-first sums over registers cost no more, so the kernel keeps them.
"""
import numpy as np
import pytest


def prefix_c(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.zeros((len(yaw), 3, 3))
    T[:, 0, 0] = c; T[:, 0, 1] = s; T[:, 1, 0] = -s; T[:, 1, 1] = c; T[:, 2, 2] = 1.0
    C = np.zeros_like(T)
    acc = np.zeros((3, 3))
    for k in range(len(yaw)):   # the serial order of the kernel
        acc = acc + T[k]
        C[k] = acc
    return C


def tables_generic(C, w):
    """The tables as the kernel formed them until round 6: every (p, q) entry a loop over i >= m of C_i - C_m."""
    N = len(C)
    W = np.diag(w)
    T1 = np.zeros((N, 3, 3)); T2 = np.zeros((N, 3, 3))
    for m in range(N):
        for i in range(m, N):
            d = C[i] - C[m]
            T1[m] += d
            T2[m] += d.T @ W @ d
    return T1, T2


def tables_six_sums(C, w):
    """The kernel's form: lane m sums t1a, t1b, t2aa, t2ab, t2bb, t2zz over i >= m from the prefix sums' two entries."""
    N = len(C)
    cc, cs = C[:, 0, 0], C[:, 0, 1]
    T1 = np.zeros((N, 3, 3)); T2 = np.zeros((N, 3, 3))
    for m in range(N):
        t1a = t1b = t2aa = t2ab = t2bb = t2zz = 0.0
        for i in range(m, N):
            da, db, dz = cc[i] - cc[m], cs[i] - cs[m], float(i - m)
            t1a += da; t1b += db
            t2aa += (w[0] * da) * da + (w[1] * db) * db
            t2ab += (w[0] * da) * db - (w[1] * db) * da
            t2bb += (w[0] * db) * db + (w[1] * da) * da
            t2zz += (w[2] * dz) * dz
        t1z = float(((N - m) * (N - m - 1)) // 2)
        T1[m] = [[t1a, t1b, 0.0], [-t1b, t1a, 0.0], [0.0, 0.0, t1z]]
        T2[m] = [[t2aa, t2ab, 0.0], [t2ab, t2bb, 0.0], [0.0, 0.0, t2zz]]
    return T1, T2


def tables_suffix(C, w):
    """Suffix-sum form, O(1) per entry: S(m) = sum_{i>=m} C_i, Q(m) = sum_{i>=m} C_i'W C_i."""
    N = len(C)
    W = np.diag(w)
    S = np.zeros((N + 1, 3, 3)); Q = np.zeros((N + 1, 3, 3))
    for m in range(N - 1, -1, -1):
        S[m] = S[m + 1] + C[m]
        Q[m] = Q[m + 1] + C[m].T @ W @ C[m]
    T1 = np.zeros((N, 3, 3)); T2 = np.zeros((N, 3, 3))
    for m in range(N):
        Cm, L = C[m], N - m
        T1[m] = S[m] - L * Cm
        T2[m] = Q[m] - Cm.T @ W @ S[m] - S[m].T @ W @ Cm + L * (Cm.T @ W @ Cm)
    return T1, T2


def yaw_cases(N, rng):
    yield "constant", np.full(N, 0.3)
    yield "zero", np.zeros(N)
    yield "ramp", 0.1 * np.arange(N) - 0.4
    for j in range(4):
        yield f"random{j}", rng.uniform(-np.pi, np.pi, N)
        yield f"slow{j}", np.cumsum(rng.normal(0.0, 0.05, N)) + rng.uniform(-1, 1)


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("N", [4, 8, 10])
def test_six_sums_equal_generic_differences_first(N):
    rng = np.random.default_rng(100 + N)
    w = np.array([4.0, 9.0, 2.5])
    for name, yaw in yaw_cases(N, rng):
        C = prefix_c(yaw)
        g1, g2 = tables_generic(C, w)
        s1, s2 = tables_six_sums(C, w)
        for m in range(N):   # entry by entry, against each step's own scale (the entries near the end are small)
            assert rel_err(s1[m], g1[m]) <= 4 * np.finfo(float).eps, (name, m)
            assert rel_err(s2[m], g2[m]) <= 4 * np.finfo(float).eps, (name, m)


@pytest.mark.parametrize("N", [4, 8, 10])
def test_suffix_form_cancels_near_the_end_of_the_horizon(N):
    rng = np.random.default_rng(200 + N)
    w = np.array([4.0, 9.0, 2.5])
    worst1 = worst2 = 0.0
    for name, yaw in yaw_cases(N, rng):
        C = prefix_c(yaw)
        g1, g2 = tables_generic(C, w)
        u1, u2 = tables_suffix(C, w)
        for m in range(N - 1):   # (m = N - 1: both tables are exactly 0 in the generic form)
            e1, e2 = rel_err(u1[m], g1[m]), rel_err(u2[m], g2[m])
            # the suffix form is right to within the parity tests' 1e-11 ...
            assert e1 <= 1e-11 and e2 <= 1e-11, (name, m, e1, e2)
            worst1, worst2 = max(worst1, e1), max(worst2, e2)
    # ... but T2 loses digits the differences-first form keeps (which is within 4 ulps of the generic form, above)
    assert worst1 <= 16 * np.finfo(float).eps
    assert worst2 > 5 * N * np.finfo(float).eps
