"""The prefix sums C_k of the one-wave set-up (csrc/srbdqp_setup1.hpp: cc_k = sum_{l<=k} cos yaw_l, cs_k = sum_{l<=k} sin yaw_l) as a chain over neighbouring
lanes -- acc = 0 + c on every lane, then N - 1 times acc = (acc of the lane before, +0.0 into lane 0) + c -- against the guarded serial loop it replaces, in which
lane m adds the terms of all N steps in ascending order, those past m selected to +0.0.  A NumPy model of the 16 lanes of a DPP row, bit for bit: the chain keeps
the loop's association ((0 + c_0) + c_1) + ..., its +0 for c_0 = -0.0 included, and a lane that is final (lane m after step m) forms the same value again in
every later step."""
import numpy as np
import pytest

ROW = 16                                     # lanes of a DPP row: row_shr:1 shifts inside it


def serial_loop(c, N):
    """lane m: acc = 0; for k < N: acc += (k <= m) ? c_k : 0.0   (c: the terms on lanes 0 .. N - 1)"""
    acc = np.zeros(ROW)
    lane = np.arange(ROW)
    for k in range(N):
        acc = acc + np.where(k <= lane, c[k], 0.0)
    return acc


def lane_chain(c_lane, N):
    """c_lane: the term every lane holds (lanes >= N: whatever the kernel left there)"""
    acc = 0.0 + c_lane
    for _ in range(1, N):
        prev = np.concatenate(([0.0], acc[:-1]))     # row_shr:1, bound_ctrl: +0.0 into the first lane
        acc = prev + c_lane
    return acc


def _check(yaw, N):
    yaw = np.asarray(yaw, dtype=np.float64)
    assert yaw.shape == (N,)
    for term in (np.cos(yaw), np.sin(yaw)):
        lanes = np.full(ROW, np.nan)                 # (lanes past N - 1 hold values nobody reads: NaN here, so that a read would show)
        lanes[:N] = term
        want = serial_loop(term, N)[:N]
        got = lane_chain(lanes, N)[:N]
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("N", [4, 8, 10])
def test_random_yaws(N):
    rng = np.random.default_rng(2300 + N)
    for _ in range(200):
        _check(rng.uniform(-np.pi, np.pi, N), N)
        _check(rng.normal(0.0, 0.3, N), N)


@pytest.mark.parametrize("N", [4, 8, 10])
def test_all_yaws_zero(N):
    _check(np.zeros(N), N)
    _check(-np.zeros(N), N)


@pytest.mark.parametrize("N", [4, 8, 10])
def test_a_first_yaw_of_minus_zero(N):
    rng = np.random.default_rng(2310 + N)
    yaw = rng.uniform(-1.0, 1.0, N)
    yaw[0] = -0.0
    assert np.signbit(np.sin(yaw[0]))                # c_0 = -0.0: the loop's 0 + c_0 is +0.0, and so is the chain's
    _check(yaw, N)
    lanes = np.zeros(ROW)
    lanes[0] = -0.0
    assert not np.signbit(lane_chain(lanes, N)[0]) and not np.signbit(serial_loop(lanes, N)[0])
    yaw[1:] = -0.0                                   # every term of the sine sum -0.0
    _check(yaw, N)


@pytest.mark.parametrize("N", [4, 8, 10])
def test_yaws_around_plus_and_minus_pi(N):
    rng = np.random.default_rng(2320 + N)
    for _ in range(200):
        sign = rng.choice([-1.0, 1.0], N)
        _check(sign * (np.pi - rng.uniform(0.0, 1e-6, N)), N)      # cos ~ -1, sin of both signs and tiny: cancellation in the sine sum
        _check(sign * np.pi, N)
