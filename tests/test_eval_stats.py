"""The statistics stages of the policy evaluator on their own: `mppo_eval_accumulate` / `mppo_eval_reduce` (csrc/k_eval.hip) on synthetic
reward / done / metrics arrays, without stepping a robot.

The metrics are what the env kernel's bookkeeping would be (oracle/env_oracle.py: metrics_step in float32) for seeded rewards and `done` draws of
probability 0 (no episode ends: +inf / -inf, every environment a survivor), 0.3 and 1 (every step ends an episode, nobody survives).  Sizes: N = 1 (a
lone thread), 70, 257 (one past a 256-thread workgroup: a second accumulate block of one thread, a second stride of the reducer for thread 0 only)
and 1100 (several strides of the reducer, the last one partial); K = 5 steps.  Exactness as in tests/test_evaluate.py: counts, min and max equal
NumPy's; the double sums within 1e-12 * sum|x| of NumPy's float64 (at most N + K additions of 2^-53 each: 1.3e-13 at N = 1100).  The trajectory
row of the same launch is checked bit for bit with a state row wider than the copied part and an odd number of recorded environments."""

import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from oracle.env_oracle import metrics_step
from physics_harness import METRIC_TYPES

f32 = np.float32
K = 5
ROW_W, STATE_LD, A, ACT_LD = 5, 11, 3, 4


def _synthetic(n, p, seed):
    r = np.random.default_rng(seed)
    reward = (3.0 * r.standard_normal((K, n))).astype(f32)
    done = (r.random((K, n)) < p).astype(np.uint8)
    m = {k: np.zeros(n, t) for k, t in METRIC_TYPES.items()}
    mets = []
    for t in range(K):
        m = metrics_step(m, reward[t], done[t], f32)
        mets.append({k: np.asarray(m[k]).astype(METRIC_TYPES[k]) for k in METRIC_TYPES})
    state = r.standard_normal((K, n, STATE_LD)).astype(f32)
    action = r.standard_normal((K, n, ACT_LD)).astype(f32)
    return reward, done, mets, state, action


def _run(be, n, p, seed=11):
    reward, done, mets, state, action = _synthetic(n, p, seed)
    Rr = min(n, 3)
    W = ROW_W + A + 2
    acc = be.full((nat.EVAL_ACC_SLOTS * n,), -7, np.int64)  # (garbage: the first step writes the accumulators without reading them)
    res = be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64)
    rows = be.full((K, Rr, W), np.nan)
    d_rew, d_done = be.zeros((n,)), be.zeros((n,), np.uint8)
    d_met = {k: be.zeros((n,), t) for k, t in METRIC_TYPES.items()}
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in d_met.items()})
    d_state, d_act = be.zeros((n, STATE_LD)), be.zeros((n, ACT_LD))
    for t in range(K):
        be.put(d_rew, reward[t]); be.put(d_done, done[t]); be.put(d_state, state[t]); be.put(d_act, action[t])
        for k in METRIC_TYPES:
            be.put(d_met[k], mets[t][k])
        row_ptr = be.ptr(rows) + t * Rr * W * 4
        be.lib.eval_accumulate(n, int(t == 0), be.ptr(d_rew), be.ptr(d_done), C.byref(M), be.ptr(acc), be.ptr(d_state), STATE_LD, ROW_W, be.ptr(d_act), ACT_LD, A, Rr,
                               row_ptr, be.stream)
        be.sync()
    be.lib.eval_reduce(n, K, be.ptr(acc), be.ptr(res), be.stream)
    be.sync()
    raw = be.host(res).tobytes()
    return nat.EvalResultRaw.from_buffer_copy(raw), raw, be.host(rows).copy(), (reward, done, mets, state, action)


@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 70, 257, 1100])
def test_accumulate_and_reduce_equal_numpy(be, n, p):
    r, raw, rows, (reward, done, mets, state, action) = _run(be, n, p)
    fin = done != 0
    rets = np.stack([m["returned_episode_returns"] for m in mets])[fin].astype(np.float64)
    lens = np.stack([m["returned_episode_lengths"] for m in mets])[fin].astype(np.int64)
    surv = ~fin.any(0)
    assert r.episodes == int(fin.sum()) and r.steps == K * n and r.survivors == int(surv.sum())
    assert fin.any() == (p > 0.0) or n == 1
    if n >= 70 and p == 0.3:
        assert r.episodes >= 1 and r.survivors >= 1  # (0.7^5 = 17 % of the environments see no episode end)
    if p == 1.0:
        assert r.episodes == K * n and r.survivors == 0
    if not fin.any():
        assert r.episodes == 0 and r.survivors == n and r.ret_min == np.inf and r.ret_max == -np.inf and (r.len_sum, r.len_min, r.len_max) == (0, 0, 0)
    else:
        assert (r.len_sum, r.len_min, r.len_max) == (int(lens.sum()), int(lens.min()), int(lens.max()))
        assert r.ret_min == rets.min() and r.ret_max == rets.max()
    sums = dict(ret_sum=rets, ret_sumsq=rets * rets, survivor_ret_sum=mets[-1]["episode_returns"].astype(np.float64)[surv], reward_sum=reward.astype(np.float64).reshape(-1))
    for k, x in sums.items():
        got, ref, scale = getattr(r, k), float(x.sum()), float(np.abs(x).sum())
        print(f"N={n} p={p} {k}: got {got!r} numpy {ref!r} |diff| {abs(got - ref):.3e} bound {1e-12 * scale:.3e}")
        assert abs(got - ref) <= 1e-12 * scale, (k, got, ref)
    # the trajectory rows of the same launches
    Rr = rows.shape[1]
    bits = lambda x: np.ascontiguousarray(x).view(np.uint8)
    assert np.array_equal(bits(rows[:, :, :ROW_W]), bits(state[:, :Rr, :ROW_W])) and np.array_equal(bits(rows[:, :, ROW_W:ROW_W + A]), bits(action[:, :Rr, :A]))
    assert np.array_equal(bits(rows[:, :, ROW_W + A]), bits(reward[:, :Rr])) and np.array_equal(rows[:, :, ROW_W + A + 1], fin[:, :Rr].astype(f32))
    # run to run: the same bytes
    assert _run(be, n, p)[1] == raw


def test_no_episode_becomes_nan_in_python(be):
    from minppo_amd.evaluate import result_from_struct

    r = _run(be, 70, 0.0)[0]
    out = result_from_struct(r)
    assert out.episodes == 0 and out.survivors == 70 and out.steps == K * 70 and out.trajectory is None
    for k in ("mean_return", "std_return", "min_return", "max_return", "mean_length", "min_length", "max_length"):
        assert np.isnan(getattr(out, k)), k
    assert out.survivor_mean_return == pytest.approx(r.survivor_ret_sum / 70) and out.mean_reward == pytest.approx(r.reward_sum / (K * 70))
    full = result_from_struct(_run(be, 70, 1.0)[0])
    assert full.episodes == K * 70 and np.isnan(full.survivor_mean_return) and full.min_length == full.max_length == full.mean_length == 1.0
    assert full.std_return >= 0 and full.min_return <= full.mean_return <= full.max_return


def test_stages_refuse_bad_arguments(be):
    n = 8
    acc, res = be.zeros((nat.EVAL_ACC_SLOTS * n,), np.int64), be.zeros((12,), np.int64)
    rew, done = be.zeros((n,)), be.zeros((n,), np.uint8)
    met = {k: be.zeros((n,), t) for k, t in METRIC_TYPES.items()}
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    with pytest.raises(nat.NativeError, match="N = 0"):
        be.lib.eval_accumulate(0, 1, be.ptr(rew), be.ptr(done), C.byref(M), be.ptr(acc), 0, 0, 0, 0, 0, 0, 0, 0, be.stream)
    with pytest.raises(nat.NativeError, match="null"):
        be.lib.eval_accumulate(n, 1, be.ptr(rew), be.ptr(done), C.byref(M), 0, 0, 0, 0, 0, 0, 0, 0, 0, be.stream)
    with pytest.raises(nat.NativeError, match="recorded environments"):
        be.lib.eval_accumulate(n, 1, be.ptr(rew), be.ptr(done), C.byref(M), be.ptr(acc), 0, 0, 0, 0, 0, 0, n + 1, 0, be.stream)
    with pytest.raises(nat.NativeError, match="null trajectory row"):
        be.lib.eval_accumulate(n, 1, be.ptr(rew), be.ptr(done), C.byref(M), be.ptr(acc), 0, 0, 0, 0, 0, 0, 2, 0, be.stream)
    with pytest.raises(nat.NativeError, match="null"):
        be.lib.eval_reduce(n, K, be.ptr(acc), 0, be.stream)
    be.lib.eval_accumulate(n, 1, be.ptr(rew), be.ptr(done), C.byref(M), be.ptr(acc), 0, 0, 0, 0, 0, 0, 0, 0, be.stream)
    be.lib.eval_reduce(n, 1, be.ptr(acc), be.ptr(res), be.stream)
    be.sync()
    r = nat.EvalResultRaw.from_buffer_copy(be.host(res).tobytes())
    assert r.steps == n and r.episodes == 0 and r.survivors == n
