"""Reward scaling (`training.normalize_rewards`; csrc/k_rewnorm.hip, mppo_reward_norm_partials / mppo_reward_norm_apply / mppo_engine_set_reward_norm,
`Trainer.reward_norm`): the rewards GAE reads are divided by the running standard deviation of the discounted return.

The oracle is the NumPy restatement below (`ref_*`): the reference has no counterpart.  The float32 recurrence `ret = ret * gamma + r` (a multiply, then an
add) and the product `r * inv_std32` are written operation by operation; the sums are float64.  The partial sums are NOT restated lane by lane (the wave's
sum is a butterfly on the device and a loop in the emulator): they are compared at the bound that holds for any order of at most 256 x 10 float64 terms,
n u sum|d| = 2560 x 1.1e-16 = 3e-13 sum|d| < 1e-12 sum|d| - and bit for bit where every term and sum is exact.

Shapes: N = 37 (part of one workgroup of 256 threads) and N = 300 (one whole workgroup and a part); T = 1, 3, 10 (a part of one chunk of eight steps, and a
chunk and a part).  Engines: synth_stompy_pro, N = 37, T = 3."""

import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd.config import make_config
from minppo_amd.train import reward_cfg
from physics_harness import METRIC_TYPES

f32, f64 = np.float32, np.float64
WG = 256  # environments of one apply workgroup (include/minppo_hip.h: mppo_reward_norm_partials = ceil(N / 256))
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
EPS = f32(1e-8)
GAMMA = f32(0.99)
SENTINEL = f32(-777.25)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------


def ref_apply(reward, done, carry, table, gamma, clip):
    """reward [T, N] float32, done [T, N] uint8, carry [N] float32, table [2] float32 -> (scaled [T, N] float32, carry' [N] float32, returns [T, N] float32).
    Per step: ret = ret * gamma (rounded) + reward (rounded); the return is recorded; then, where done, ret = 0."""
    T, N = reward.shape
    g = f32(gamma)
    ret = carry.astype(f32).copy()
    rets = np.empty((T, N), f32)
    for t in range(T):
        prod = ret * g
        assert prod.dtype == f32
        ret = prod + reward[t]
        assert ret.dtype == f32
        rets[t] = ret
        ret = np.where(done[t] != 0, f32(0), ret)
    scaled = reward * f32(table[1])
    assert scaled.dtype == f32
    if clip > 0:
        scaled = np.clip(scaled, f32(-clip), f32(clip))
    return scaled, ret, rets


def ref_partials(rets, mean32):
    """-> ([G, 2] float64, sum |d| per workgroup): S1 = sum d, S2 = sum d^2 over the workgroup's environments, d = (double)ret - (double)mean32; a thread's
    steps in t order, the threads by NumPy's sum."""
    T, N = rets.shape
    G = -(-N // WG)
    out, mag = np.zeros((G, 2), f64), np.zeros(G, f64)
    d = rets.astype(f64) - f64(f32(mean32))
    s1, s2 = np.zeros(N, f64), np.zeros(N, f64)
    for t in range(T):
        s1 += d[t]
        s2 += d[t] * d[t]
    for g in range(G):
        out[g, 0], out[g, 1] = s1[g * WG:(g + 1) * WG].sum(), s2[g * WG:(g + 1) * WG].sum()
        mag[g] = np.abs(d[:, g * WG:(g + 1) * WG]).sum()
    return out, mag


def ref_update(partials, rows, stats, table_mean32, eps, O):
    """tests/test_obs_norm.py ref_update (copied): partials [P, 2, O]; stats [1 + 2 O] = n | mean | M2 -> (stats', table' [2, O] float32): index-order sums,
    Chan's merge, the table."""
    n, mu, M2 = stats[0], stats[1:1 + O].copy(), stats[1 + O:].copy()
    n1 = n
    if rows > 0:
        S1, S2 = np.zeros(O, f64), np.zeros(O, f64)
        for p in partials:
            S1 = S1 + p[0]
            S2 = S2 + p[1]
        k = f64(rows)
        b = table_mean32.astype(f64) + S1 / k
        M2b = np.maximum(S2 - S1 * S1 / k, 0.0)
        delta = b - mu
        n1 = n + k
        mu = mu + delta * k / n1
        M2 = M2 + M2b + delta * delta * n * k / n1
    if n1 > 0:
        table = np.stack([mu.astype(f32), (1.0 / np.sqrt(M2 / n1 + f64(eps))).astype(f32)])
    else:
        table = np.stack([np.zeros(O, f32), np.ones(O, f32)])
    return np.concatenate([[n1], mu, M2]), table


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (np.sign(a) == np.sign(b)).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


# ---- 1 - 5: the stage ----------------------------------------------------------------------------------------------------------------------------


def _run_apply(be, reward, done, carry, table, gamma, clip, with_partials=True, in_place=False):
    """-> (scaled [T, N], carry' [N], partials [G, 2] or None).  Every output buffer is one slab longer than a launch may touch (a step's row of the
    scaled rewards, N carries, one workgroup's partials), filled with a sentinel / NaN that must survive."""
    T, N = reward.shape
    G = be.lib.reward_norm_partials(N)
    assert G == -(-N // WG)
    rew_h = np.full((T + 1, N), SENTINEL, f32)
    rew_h[:T] = reward
    car_h = np.full(2 * N, SENTINEL, f32)
    car_h[:N] = carry
    rew, dn, car, tab = be.arr(rew_h), be.arr(np.ascontiguousarray(done, np.uint8)), be.arr(car_h), be.arr(np.asarray(table, f32))
    out = rew if in_place else be.full((T + 1, N), np.nan)
    part = be.full((G + 1, 2), np.nan, f64) if with_partials else None
    be.lib.reward_norm_apply(T, N, float(gamma), be.ptr(rew), be.ptr(dn), be.ptr(car), be.ptr(tab), float(clip), be.ptr(out), be.ptr(part), be.stream)
    be.sync()
    o, c = be.host(out), be.host(car)
    assert (o[T] == SENTINEL).all() if in_place else np.isnan(o[T]).all(), "a write beyond the T x N scaled rewards"
    assert (c[N:] == SENTINEL).all(), "a write beyond the N carries"
    if not in_place:
        assert np.array_equal(_bits(be.host(rew)), _bits(rew_h)), "the rewards were written"
    assert np.array_equal(be.host(tab), np.asarray(table, f32)) and np.array_equal(be.host(dn), np.asarray(done, np.uint8))
    p = None
    if with_partials:
        p = be.host(part)
        assert np.isnan(p[G]).all(), "a write beyond the launch's partials"
        p = p[:G].copy()
    return o[:T].copy(), c[:N].copy(), p


_DONE_PATTERNS = ("random", "last_step", "every_step")


def _inputs(N, T, pattern):
    rng = np.random.default_rng(1000 * N + 10 * T + _DONE_PATTERNS.index(pattern))
    reward = (rng.standard_normal((T, N)) * 1.5 + 0.4).astype(f32)
    if pattern == "random":
        done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    elif pattern == "last_step":
        done = np.zeros((T, N), np.uint8)
        done[T - 1] = 1
    else:
        done = np.ones((T, N), np.uint8)
    carry = (rng.standard_normal(N) * 3.0).astype(f32)
    assert (carry != 0).all()
    return reward, done, carry


TABLE = np.array([0.3, 0.7], f32)
SHAPES = [(37, 1), (37, 3), (37, 10), (300, 1), (300, 3), (300, 10)]
_STAGE = {}


def _stage(be, N, T, pattern, clip):
    """The kernel's outputs on the inputs of test 1 (shared by tests 1, 3 and 4)."""
    key = (be.name, N, T, pattern, clip)
    if key not in _STAGE:
        reward, done, carry = _inputs(N, T, pattern)
        _STAGE[key] = _run_apply(be, reward, done, carry, TABLE, GAMMA, clip)
    return _STAGE[key]


@pytest.mark.parametrize("pattern", _DONE_PATTERNS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_scaled_rewards_and_carry_are_the_float32_expressions_bit_for_bit(be, N, T, pattern):
    reward, done, carry = _inputs(N, T, pattern)
    for clip in (0.0, 1.5):
        want_s, want_c, _ = ref_apply(reward, done, carry, TABLE, GAMMA, clip)
        if clip > 0:
            raw = reward * TABLE[1]
            if raw.size >= 37:  # (every shape here: some elements clamp, others do not)
                assert (np.abs(raw) > clip).any() and (np.abs(raw) < clip).any()
        got_s, got_c, part = _stage(be, N, T, pattern, clip)
        assert np.array_equal(_bits(got_s), _bits(want_s)), f"scaled, clip {clip}"
        assert np.array_equal(_bits(got_c), _bits(want_c)), f"carry, clip {clip}"
        if clip > 0:
            assert np.abs(got_s).max() == f32(clip), "the clamp value is attained"
        if pattern == "last_step" or pattern == "every_step":
            assert (got_c == 0).all(), "a carry survived the episode's end"
        else:
            assert (got_c != 0).any()
        # in place (scaled == reward): the same bytes
        in_s, in_c, in_p = _run_apply(be, reward, done, carry, TABLE, GAMMA, clip, in_place=True)
        assert np.array_equal(_bits(in_s), _bits(got_s)) and np.array_equal(_bits(in_c), _bits(got_c)) and np.array_equal(_bits(in_p), _bits(part))
        # partial = NULL: the same rewards and carry
        n_s, n_c, none = _run_apply(be, reward, done, carry, TABLE, GAMMA, clip, with_partials=False)
        assert none is None and np.array_equal(_bits(n_s), _bits(got_s)) and np.array_equal(_bits(n_c), _bits(got_c))


def test_a_nan_reward_stays_a_nan_under_the_clamp(be):
    reward, done, carry = _inputs(37, 3, "random")
    reward[1, 5] = np.nan
    got_s, got_c, _ = _run_apply(be, reward, done, carry, TABLE, GAMMA, 1.5)
    assert np.isnan(got_s[1, 5]) and np.isnan(got_s).sum() == 1


@pytest.mark.parametrize("N,T", [(37, 1), (37, 3), (37, 6), (300, 1), (300, 3), (300, 6)])
def test_partials_are_exact_on_dyadic_inputs(be, N, T):
    """Rewards on the grid of multiples of 2^-4 within +-4, gamma = 0.5, carry 0, mean 0.375: after at most 6 steps a return is a multiple of 2^-9 below 8
    in magnitude (exact in float32, so the recurrence rounds nowhere), d a multiple of 2^-9 below 8.375, d^2 a multiple of 2^-18 below 71, and every sum over
    256 x 6 of them is exact in float64 in any order: the partials must EQUAL the float64 sums."""
    rng = np.random.default_rng(N + T)
    reward = (rng.integers(-64, 65, (T, N)) / 16.0).astype(f32)
    done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    table = np.array([0.375, 0.5], f32)
    scaled, carry, part = _run_apply(be, reward, done, np.zeros(N, f32), table, 0.5, 0.0)
    want_s, want_c, rets = ref_apply(reward, done, np.zeros(N, f32), table, 0.5, 0.0)
    assert np.array_equal(_bits(scaled), _bits(want_s)) and np.array_equal(_bits(carry), _bits(want_c))
    G = -(-N // WG)
    d = rets.astype(f64) - 0.375
    assert part.shape == (G, 2)
    for g in range(G):
        grp = d[:, g * WG:(g + 1) * WG]
        assert part[g, 0] == grp.sum() and part[g, 1] == (grp * grp).sum(), g
    assert np.array_equal(part, ref_partials(rets, table[0])[0])  # (and the restatement is those sums)
    # nothing of an environment beyond N: with one environment more in the arrays (row stride N + 1 would be another layout, so: N - 1 of these N)
    s2, c2, p2 = _run_apply(be, np.ascontiguousarray(reward[:, :N - 1]), np.ascontiguousarray(done[:, :N - 1]), np.zeros(N - 1, f32), table, 0.5, 0.0)
    d2 = d[:, :N - 1]
    for g in range(-(-(N - 1) // WG)):
        grp = d2[:, g * WG:(g + 1) * WG]
        assert p2[g, 0] == grp.sum() and p2[g, 1] == (grp * grp).sum(), g


@pytest.mark.parametrize("pattern", _DONE_PATTERNS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_partials_on_general_inputs(be, N, T, pattern):
    """The inputs of test 1.  Any order of at most 256 x 10 float64 additions is within n u sum|d| = 3e-13 sum|d| of the exact sum (and of the
    restatement's): S1 at atol 1e-12 sum|d| (it may cancel), S2, a sum of non-negative terms, at rtol 1e-12.  The clamp does not touch them."""
    reward, done, carry = _inputs(N, T, pattern)
    _, _, rets = ref_apply(reward, done, carry, TABLE, GAMMA, 0.0)
    want, mag = ref_partials(rets, TABLE[0])
    for clip in (0.0, 1.5):
        part = _stage(be, N, T, pattern, clip)[2]
        assert part.shape == want.shape
        for g in range(len(want)):
            print(f"N {N} T {T} {pattern} clip {clip} wg {g}: S1 {part[g, 0]!r} want {want[g, 0]!r} |diff| / sum|d| {abs(part[g, 0] - want[g, 0]) / mag[g]:.2e}; "
                  f"S2 {part[g, 1]!r} want {want[g, 1]!r} rel {abs(part[g, 1] - want[g, 1]) / want[g, 1]:.2e}")
            assert abs(part[g, 0] - want[g, 0]) <= 1e-12 * mag[g]
        np.testing.assert_allclose(part[:, 1], want[:, 1], rtol=1e-12, atol=0)
    assert np.array_equal(_bits(_stage(be, N, T, pattern, 0.0)[2]), _bits(_stage(be, N, T, pattern, 1.5)[2]))
    # the same inputs, the same bytes
    again = _run_apply(be, reward, done, carry, TABLE, GAMMA, 0.0)[2]
    assert np.array_equal(_bits(again), _bits(_stage(be, N, T, pattern, 0.0)[2]))


def _run_update(be, partials, rows, stats, table, eps=EPS):
    """mppo_obs_norm_update with O = 1 and table_ld = 1 on [G][2] partials -> (stats [3], table [2])."""
    sdev, tdev, pdev = be.arr(np.asarray(stats, f64)), be.arr(np.asarray(table, f32)), be.arr(np.asarray(partials, f64))
    be.lib.obs_norm_update(1, len(partials), int(rows), be.ptr(pdev), be.ptr(sdev), float(eps), be.ptr(tdev), 1, be.stream)
    be.sync()
    return be.host(sdev).copy(), be.host(tdev).copy()


@pytest.mark.parametrize("stats0", [(0.0, 0.0, 0.0), (5000.0, 1.25, 5000.0 * 7.5)], ids=["from_zero", "from_statistics"])
@pytest.mark.parametrize("N,T", [(37, 3), (300, 10)])
def test_the_merge_is_obs_norm_update_with_one_column(be, N, T, stats0):
    """The kernel's own partials of test 1 merged by mppo_obs_norm_update(1, G, T N, ..., table_ld = 1) against the restatement: the statistics at rtol
    1e-14 (a dozen float64 operations), the table within one float32 ulp."""
    part = _stage(be, N, T, "random", 0.0)[2]
    got_stats, got_table = _run_update(be, part, T * N, stats0, TABLE)
    want_stats, want_table = ref_update(part.reshape(-1, 2, 1), T * N, np.array(stats0, f64), TABLE[:1], EPS, 1)
    assert got_stats.shape == (3,) and got_table.shape == (2,) and got_stats[0] == stats0[0] + T * N
    np.testing.assert_allclose(got_stats, want_stats, rtol=1e-14, atol=0)
    assert _ulps(got_table, want_table.reshape(2)) <= 1
    # and they are the statistics of the returns themselves
    reward, done, carry = _inputs(N, T, "random")
    rets = ref_apply(reward, done, carry, TABLE, GAMMA, 0.0)[2].astype(f64)
    if stats0[0] == 0:
        np.testing.assert_allclose(got_stats[1], rets.mean(), rtol=1e-12)
        np.testing.assert_allclose(got_stats[2] / got_stats[0], rets.var(), rtol=1e-12)


def test_a_constant_reward_gives_a_finite_scale(be):
    """gamma = 0: the return is the reward, 0.5 everywhere; S1 = k / 2, S2 = k / 4 exactly, M2 = 0, scale = float32(1 / sqrt(eps)) - finite."""
    N, T = 300, 3
    ident = np.array([0.0, 1.0], f32)
    reward, done = np.full((T, N), 0.5, f32), np.zeros((T, N), np.uint8)
    scaled, carry, part = _run_apply(be, reward, done, np.zeros(N, f32), ident, 0.0, 0.0)
    assert (scaled == 0.5).all() and (carry == 0.5).all()
    stats, table = _run_update(be, part, T * N, np.zeros(3), ident)
    assert stats[0] == T * N and stats[1] == 0.5 and stats[2] == 0.0
    assert table[0] == f32(0.5) and table[1] == f32(1.0 / np.sqrt(f64(EPS))) and np.isfinite(table).all()
    scaled, _, _ = _run_apply(be, reward, done, np.zeros(N, f32), table, 0.0, 10.0)
    assert np.isfinite(scaled).all() and (scaled == 10.0).all()


def test_apply_refuses_bad_arguments(be):
    f = be.lib._fn["mppo_reward_norm_apply"]
    T, N = 3, 8
    rew, dn, car, tab, out, part = be.zeros((T, N)), be.zeros((T, N), np.uint8), be.zeros((N,)), be.arr(np.array([0, 1], f32)), be.zeros((T, N)), be.zeros((1, 2), f64)
    p = be.ptr
    g = float(GAMMA)
    assert f(T, N, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), p(part), be.stream) == 0
    assert f(T, N, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), None, be.stream) == 0
    be.sync()
    assert f(T, N, g, p(rew), p(dn), p(car), p(tab), -1.0, p(out), p(part), be.stream) == -1 and "negative" in be.lib.last_error()
    assert f(T, N, g, p(rew), p(dn), p(car), p(tab), float("nan"), p(out), p(part), be.stream) == -1 and "clip" in be.lib.last_error()
    assert f(0, N, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), p(part), be.stream) == -1 and "T = 0" in be.lib.last_error()
    assert f(-1, N, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), p(part), be.stream) == -1
    assert f(T, 0, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), p(part), be.stream) == -1 and "N = 0" in be.lib.last_error()
    assert f(T, -5, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), p(part), be.stream) == -1
    for k in range(5):  # reward, done, carry, table, scaled: each of them null
        ptrs = [p(rew), p(dn), p(car), p(tab), p(out)]
        ptrs[k] = None
        assert f(T, N, g, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 0.0, ptrs[4], p(part), be.stream) == -1 and "null" in be.lib.last_error(), k
    assert f(T, N, g, p(rew) + 2, p(dn), p(car), p(tab), 0.0, p(out), p(part), be.stream) == -1 and "aligned" in be.lib.last_error()
    assert f(T, N, g, p(rew), p(dn), p(car), p(tab), 0.0, p(out), p(part) + 4, be.stream) == -1 and "aligned" in be.lib.last_error()
    assert be.lib.reward_norm_partials(0) == 0 and be.lib.reward_norm_partials(-3) == 0 and be.lib.reward_norm_partials(256) == 1
    assert be.lib.reward_norm_partials(257) == 2 and be.lib.reward_norm_partials(4096) == 16


# ---- 6 - 10: the engine ----------------------------------------------------------------------------------------------------------------------------

NE, TE = 37, 3
ENGINE = [f"training.num_envs={NE}", f"training.num_steps={TE}", f"rl.num_env_steps={TE}", "training.num_minibatches=3", "training.update_epochs=1",
          "model.hidden_size=32", f"training.total_timesteps={NE * TE * 8}"]
# a height window that ends episodes at every step (tests/test_obs_norm.py): the carry then restarts in some environments and not in others
FALLING = ["environment.reset_noise_scale=0.01", "reward.height_min_z=1.005", "reward.height_max_z=1.012"]
NORM = ["training.normalize_rewards=true", "training.reward_norm_clip=0"]
NEW_REGIONS = ("reward_norm_stats", "reward_norm_table", "reward_norm_carry", "reward_norm_partials", "reward_scaled")


def _host(tr, name, shape=None):
    return np.array(tr._to_host(tr.region(name, shape)))


def test_first_rollout_is_the_plain_engines(be):
    """The scale is 1 until the first rollout's merge has run: r * 1.0f == r, so the scaling engine's first rollout leaves the plain engine's bytes, and
    its statistics are the restatement over the T N discounted returns from a zero carry."""
    plain = be.trainer(make_config(BASE, ENGINE + FALLING))
    norm = be.trainer(make_config(BASE, ENGINE + FALLING + NORM))
    for tr in (plain, norm):
        tr.reset()
    norm._sync()
    assert (_host(norm, "reward_norm_stats") == 0).all() and (_host(norm, "reward_norm_carry") == 0).all()
    assert np.array_equal(_host(norm, "reward_norm_table"), np.array([0, 1], f32))
    assert norm.reward_norm()["count"] == 0 and norm.reward_norm()["scale"] == 1.0
    for tr in (plain, norm):
        tr.rollout()
        tr._sync()
    for name in ("obs", "action", "reward", "done", "value", "log_prob", "adv", "target", "last_val", "rollout_stats"):
        assert np.array_equal(_bits(_host(plain, name)), _bits(_host(norm, name))), name
    reward, done = _host(norm, "reward", (TE, NE)), _host(norm, "done", (TE, NE))
    assert done.any() and not done.all(), "the window must end some episodes: the carry restarts there"
    assert np.array_equal(_bits(_host(norm, "reward_scaled", (TE, NE))), _bits(reward))
    gamma = f32(norm.config.rl.gamma)
    _, want_carry, rets = ref_apply(reward, done, np.zeros(NE, f32), np.array([0, 1], f32), gamma, 0.0)
    assert np.array_equal(_bits(_host(norm, "reward_norm_carry")), _bits(want_carry))
    part = _host(norm, "reward_norm_partials", (1, 2))
    want_part, mag = ref_partials(rets, f32(0))
    assert abs(part[0, 0] - want_part[0, 0]) <= 1e-12 * mag[0]
    np.testing.assert_allclose(part[:, 1], want_part[:, 1], rtol=1e-12, atol=0)
    want_stats, want_table = ref_update(part.reshape(-1, 2, 1), TE * NE, np.zeros(3), np.zeros(1, f32), f32(norm.config.training.reward_norm_eps), 1)
    got = _host(norm, "reward_norm_stats")
    assert got[0] == TE * NE
    np.testing.assert_allclose(got, want_stats, rtol=1e-14, atol=0)
    np.testing.assert_allclose(got[1], rets.astype(f64).mean(), rtol=1e-11)
    np.testing.assert_allclose(got[2] / got[0], rets.astype(f64).var(), rtol=1e-11)
    table = _host(norm, "reward_norm_table")
    assert _ulps(table, want_table.reshape(2)) <= 1 and table[1] != 1
    rn = norm.reward_norm()
    assert set(rn) == {"count", "mean", "var", "scale", "clip", "eps"}
    assert rn["count"] == TE * NE and rn["scale"] == float(table[1]) and rn["mean"] == got[1] and rn["var"] == got[2] / got[0] and rn["clip"] == 0.0
    assert rn["eps"] == pytest.approx(1e-8)
    # the plain engine's regions are there and untouched (its arena starts zeroed)
    for name in NEW_REGIONS:
        assert (_host(plain, name) == 0).all(), name
    assert plain.reward_norm()["count"] == 0 and plain.reward_norm()["scale"] == 1.0
    plain.close(); norm.close()


def _write_random(be, tr, rng):
    noise = rng.standard_normal((tr.T, tr.N, tr.A)).astype(f32)
    perms = np.stack([rng.permutation(tr.N * tr.T) for _ in range(tr.E)]).astype(np.int32)
    be.put(tr.region("noise", (tr.T, tr.N, tr.A)), noise)
    be.put(tr.region("perm", (tr.E, tr.N * tr.T)), perms)
    return noise


@pytest.mark.parametrize("extra", [[], ["training.reward_norm_clip=0.5"]], ids=["no_clip", "clip"])
def test_second_rollout_equals_the_composition_of_the_stages(be, extra):
    """Update 2's rollout written out with the ABI's own stages - mppo_policy_forward, mppo_env_step (and the reset noise's mppo_env_reinit, event
    u T + 1 + t of update u = 1) per step, the bootstrap mppo_policy_forward, mppo_reward_norm_apply, mppo_gae on the scaled rewards,
    mppo_obs_norm_update - from the engine's state, parameters, carry, statistics and table after update 1: bit for bit.  (Noise and permutations are
    written by the test: external_random.)"""
    cfg = make_config(BASE, ENGINE + FALLING + NORM + extra)
    clip = float(cfg.training.reward_norm_clip)
    tr = be.trainer(cfg, external_random=True)
    tr.reset()
    rng = np.random.default_rng(11)
    _write_random(be, tr, rng)
    tr.update()
    tr._sync()
    N, Tn, O, OP, A = tr.N, tr.T, tr.O, tr.OP, tr.A
    host = lambda name, shape=None: _host(tr, name, shape)
    stats1, table1, carry1 = host("reward_norm_stats"), host("reward_norm_table"), host("reward_norm_carry")
    assert stats1[0] == Tn * N and table1[1] != 1 and np.isfinite(table1).all()
    state, rec, params = be.arr(host("state", (N, tr.dims.rec_dim))), be.arr(host("reset_rec")), be.arr(host("params"))
    obs = be.arr(host("obs", (Tn + 1, N, OP)))  # slot 0: update 1's last row
    met = {k: be.arr(host(k).astype(t)) for k, t in METRIC_TYPES.items()}
    noise = _write_random(be, tr, rng)
    tr.rollout()
    tr._sync()
    # ---- the replay
    lib, s = be.lib, be.stream
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    noise_d = be.arr(noise)
    act, logp, val, last = be.zeros((Tn, N, A)), be.zeros((Tn, N)), be.zeros((Tn, N)), be.zeros((N,))
    rew, done, scaled, adv, target = be.zeros((Tn, N)), be.zeros((Tn, N), np.uint8), be.zeros((Tn, N)), be.zeros((Tn, N)), be.zeros((Tn, N))
    wsb = lib.policy_ws_bytes(C.byref(tr.net), N)
    ws = be.zeros((wsb,), np.uint8)
    G = lib.reward_norm_partials(N)
    part, sdev, tdev, cdev = be.zeros((G, 2), f64), be.arr(stats1), be.arr(table1), be.arr(carry1)
    rc = reward_cfg(cfg)
    row, arow = N * OP * 4, N * A * 4
    gamma, lam = float(f32(cfg.rl.gamma)), float(f32(cfg.rl.gae_lambda))
    for t in range(Tn):
        lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + t * row, OP, be.ptr(noise_d) + t * arow, be.ptr(act) + t * arow,
                           be.ptr(logp) + t * N * 4, be.ptr(val) + t * N * 4, 0, be.ptr(ws), wsb, s)
        lib.env_step(tr._model, N, cfg.environment.n_frames, C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(act) + t * arow, A, be.ptr(obs) + (t + 1) * row, OP,
                     be.ptr(rew) + t * N * 4, be.ptr(done) + t * N, C.byref(M), s)
        lib.env_reinit(tr._model, N, be.ptr(state), be.ptr(obs) + (t + 1) * row, OP, be.ptr(done) + t * N, float(cfg.environment.reset_noise_scale), 0, int(tr.seed), 0,
                       0, 0, Tn + 1 + t, s)
    lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + Tn * row, OP, 0, 0, 0, be.ptr(last), 0, be.ptr(ws), wsb, s)
    lib.reward_norm_apply(Tn, N, gamma, be.ptr(rew), be.ptr(done), be.ptr(cdev), be.ptr(tdev), clip, be.ptr(scaled), be.ptr(part), s)
    lib.gae(Tn, N, gamma, lam, be.ptr(scaled), be.ptr(val), be.ptr(done), be.ptr(last), be.ptr(adv), be.ptr(target), s)
    lib.obs_norm_update(1, G, Tn * N, be.ptr(part), be.ptr(sdev), float(cfg.training.reward_norm_eps), be.ptr(tdev), 1, s)
    be.sync()
    for name, mine in (("obs", obs), ("reward", rew), ("done", done), ("value", val), ("reward_scaled", scaled), ("adv", adv), ("target", target), ("reward_norm_carry", cdev),
                       ("reward_norm_partials", part), ("reward_norm_stats", sdev), ("reward_norm_table", tdev)):
        assert np.array_equal(_bits(host(name)).reshape(-1), _bits(be.host(mine)).reshape(-1)), name
    assert host("reward_norm_stats")[0] == 2 * Tn * N
    raw, sc, dn = host("reward", (Tn, N)), host("reward_scaled", (Tn, N)), host("done", (Tn, N))
    assert dn.any() and not dn.all()
    assert not np.array_equal(sc, raw), "the scale moved off 1"
    want = ref_apply(raw, dn, carry1, table1, f32(cfg.rl.gamma), clip)
    assert np.array_equal(_bits(sc), _bits(want[0])) and np.array_equal(_bits(host("reward_norm_carry")), _bits(want[1]))
    if clip > 0:
        assert np.abs(sc).max() == f32(clip), "the scaled rewards are clamped"
    # the statistics users see are those of the raw rewards
    assert host("rollout_stats")[0] == pytest.approx(raw.astype(f64).sum(), rel=1e-6)
    assert abs(host("rollout_stats")[0] - sc.astype(f64).sum()) > 1e-3 * np.abs(raw).astype(f64).sum()
    tr.close()


def test_set_reward_norm_state_rules(be):
    cfg = make_config(BASE, ENGINE)
    f = be.lib._fn["mppo_engine_set_reward_norm"]
    tr = be.trainer(cfg)
    assert f(tr._engine, 1, -1.0, 1e-8) == -1 and "negative" in be.lib.last_error()  # MPPO_EINVAL
    assert f(tr._engine, 1, 10.0, -1e-8) == -1 and f(tr._engine, 1, float("nan"), 1e-8) == -1 and f(tr._engine, 1, 10.0, float("nan")) == -1
    be.lib.engine_set_reward_norm(tr._engine, 1, 10.0, 1e-8)
    be.lib.engine_set_reward_norm(tr._engine, 0, 0.0, 0.0)
    tr.reset()
    assert f(tr._engine, 1, 10.0, 1e-8) == -4 and "mppo_engine_reset has run" in be.lib.last_error()  # MPPO_ESTATE
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert f(tr._engine, 1, 10.0, 1e-8) == -4 and "prepared" in be.lib.last_error()
    with pytest.raises(nat.NativeError):
        be.lib.engine_set_reward_norm(tr._engine, 0, 0.0, 0.0)
    tr.close()
    # several ranks: refused by the engine (the message names the ranks) and, before anything is created, by the Trainer
    even = [x for x in ENGINE if "num_envs" not in x and "minibatches" not in x] + ["training.num_envs=32", "training.num_minibatches=2"]
    two = be.trainer(make_config(BASE, even), world_size=2, rank=0)
    assert f(two._engine, 1, 10.0, 1e-8) == -1 and "world_size = 2 ranks" in be.lib.last_error()
    be.lib.engine_set_reward_norm(two._engine, 0, 10.0, 1e-8)  # (switching it off is nothing a rank count forbids)
    two.close()
    with pytest.raises(ValueError, match="2 ranks"):
        be.trainer(make_config(BASE, even + ["training.normalize_rewards=true"]), world_size=2, rank=0)


def test_graph_replay_equals_eager_launches(be):
    """Three updates replayed from the captured graph and launched eagerly: the same parameters, statistics, table and carry (on the emulator both are
    eager)."""
    cfg = make_config(BASE, ENGINE + NORM[:1] + FALLING)
    out = {}
    for graph in (True, False):
        tr = be.trainer(cfg, use_graph=graph)
        tr.reset()
        for _ in range(3):
            tr.update()
        tr._sync()
        if be.name == "hip":
            assert tr.graph_active() == graph
        out[graph] = {n: _host(tr, n) for n in ("params", "reward_norm_stats", "reward_norm_table", "reward_norm_carry")}
        assert out[graph]["reward_norm_stats"][0] == 3 * TE * NE and tr.reward_norm()["count"] == 3 * TE * NE
        assert np.isfinite(out[graph]["params"]).all() and out[graph]["reward_norm_table"][1] != 1
        tr.close()
    for n in out[True]:
        assert np.array_equal(_bits(out[True][n]), _bits(out[False][n])), n


def test_together_with_observation_normalisation_and_reset_noise(be):
    cfg = make_config(BASE, ENGINE + FALLING + ["training.normalize_rewards=true", "training.normalize_observations=true"])
    tr = be.trainer(cfg)
    tr.reset()
    tr.update(); tr.update()
    tr._sync()
    for name in ("params", "obs", "reward", "reward_scaled", "adv", "target", "reward_norm_stats", "reward_norm_table", "reward_norm_carry", "obs_norm_stats",
                 "obs_norm_table"):
        assert np.isfinite(_host(tr, name)).all(), name
    assert np.isfinite(tr.losses()).all()
    assert tr.reward_norm()["count"] == tr.obs_norm()["count"] == 2 * TE * NE
    assert tr.reward_norm()["scale"] != 1.0 and tr.reward_norm()["clip"] == 10.0
    tr.close()


# ---- 11, 12: the Python layer ------------------------------------------------------------------------------------------------------------------------


def test_checkpoint_resume_is_bit_exact_and_refuses_the_other_setting(be, tmp_path):
    over = ["training.num_envs=24", "training.num_steps=3", "rl.num_env_steps=3", "training.num_minibatches=2", "training.update_epochs=1", "model.hidden_size=32",
            "training.total_timesteps=100000"] + FALLING + ["training.normalize_rewards=true"]
    cfg = make_config(BASE, over)
    ck = str(tmp_path / "ck" / "state.npz")
    names = ("params", "adam_m", "state", "reward_norm_stats", "reward_norm_table", "reward_norm_carry")
    a = be.trainer(cfg)
    a.reset()
    a.update(); a.update()
    a.save_checkpoint(ck)
    a.update(); a.update()
    a._sync()
    want = {n: _host(a, n) for n in names}
    a.close()
    b = be.trainer(cfg)
    b.load_checkpoint(ck)
    assert b.updates_done == 2 and b.reward_norm()["count"] == 2 * 3 * 24 and b.reward_norm()["scale"] != 1.0
    assert _host(b, "reward_norm_carry").any(), "the carried returns came back"
    b.update(); b.update()
    b._sync()
    for n in names:
        assert np.array_equal(_bits(_host(b, n)), _bits(want[n])), n
    assert b.reward_norm()["count"] == 4 * 3 * 24
    b.close()
    c = be.trainer(make_config(BASE, over[:-1]))
    with pytest.raises(ValueError, match=r"normalize_rewards=true.*normalize_rewards=false"):
        c.load_checkpoint(ck)
    c.reset()
    c.update()
    c._sync()
    ck2 = str(tmp_path / "ck" / "plain.npz")
    c.save_checkpoint(ck2)
    want_c = {n: _host(c, n) for n in ("params", "adam_m", "state")}
    c.close()
    d = be.trainer(cfg)
    with pytest.raises(ValueError, match=r"normalize_rewards=false.*normalize_rewards=true"):
        d.load_checkpoint(ck2)
    d.close()
    # a checkpoint written by a plain trainer still loads into a plain trainer
    e = be.trainer(make_config(BASE, over[:-1]))
    e.load_checkpoint(ck2)
    e._sync()
    assert e.updates_done == 1
    for n, w in want_c.items():
        assert np.array_equal(_bits(_host(e, n)), _bits(w)), n
    for name in NEW_REGIONS:
        assert (_host(e, name) == 0).all(), name
    e.close()


def test_config_keys():
    tr = make_config(BASE).training
    assert tr.normalize_rewards is False and tr.reward_norm_clip == 10.0 and tr.reward_norm_eps == 1e-8
    tr = make_config(BASE, ["training.normalize_rewards=true", "training.reward_norm_clip=0", "training.reward_norm_eps=1e-6"]).training
    assert tr.normalize_rewards is True and tr.reward_norm_clip == 0.0 and tr.reward_norm_eps == pytest.approx(1e-6)
    assert make_config({**BASE, "training": {"normalize_rewards": True, "reward_norm_clip": 5}}).training.reward_norm_clip == 5.0
    assert make_config({**BASE, "training": {"normalize_rewards": True}}).training.normalize_rewards is True
    with pytest.raises(ValueError, match="reward_norm_clip"):
        make_config(BASE, ["training.reward_norm_clip=-1"])
    with pytest.raises(ValueError, match="reward_norm_eps"):
        make_config(BASE, ["training.reward_norm_eps=-1e-8"])
