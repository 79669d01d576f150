"""Running observation normalisation (`training.normalize_observations`; csrc/k_obsnorm.hip, mppo_obs_norm_* / mppo_engine_set_obs_norm /
mppo_evaluate_obs_norm, `Trainer.obs_norm`, the "obs_norm" entry of the model file).

The oracle is the float64 NumPy restatement below (`ref_*`): the reference has no counterpart.  It restates the kernels' ORDER too - a workgroup's 128
rows in groups of eight, each in row order, the groups' sums in row order, the partials in index order, the merge operation by operation - so that the float64 sums it is compared with at rtol 1e-14 are the
same sums (a mean that cancels to nearly zero has no relative accuracy under any other order).

Shapes: O = 225 / obs_ld = 228 (the flagship observation: 56 whole 16-byte units and one that reaches into the pad) and O = 7 / obs_ld = 8; N = 37 (part of
one workgroup of 128 rows: four whole waves of eight rows, a part of the fifth, eleven idle) and N = 300 (two workgroups and a part); unaligned / odd strides for the one-column form.  Engines: synth_stompy_pro,
N = 37, T = 3."""

import ctypes as C
import pickle

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd import train as T
from minppo_amd.config import make_config
from minppo_amd.evaluate import evaluate
from minppo_amd.model import load_model
from minppo_amd.train import init_flat_params, reward_cfg
from physics_harness import METRIC_TYPES

f32, f64 = np.float32, np.float64
ROWS, GROUP = 128, 8  # rows of one apply workgroup, and of one of its 16 waves (include/minppo_hip.h: mppo_obs_norm_partials = ceil(N / 128))
BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
EPS = f32(1e-8)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------


def ref_apply(x, table, clip):
    """x [N, O] float32, table [2, O] float32 -> y float32: (x - m) * s in float32 in that order, then the clamp."""
    y = (x - table[0][None, :]) * table[1][None, :]
    assert y.dtype == f32
    return np.clip(y, f32(-clip), f32(clip)) if clip > 0 else y


def ref_partials(x, mean32):
    """-> [G, 2, O] float64: per workgroup of 128 rows S1 = sum d, S2 = sum d^2, d = (double)x - (double)mean32: every group of 8 rows in row order,
    then the groups' sums in row order."""
    N, O = x.shape
    G = -(-N // ROWS)
    out = np.zeros((G, 2, O), f64)
    for g in range(G):
        for w0 in range(g * ROWS, (g + 1) * ROWS, GROUP):
            grp = np.zeros((2, O), f64)
            for r in range(w0, min(N, w0 + GROUP)):
                d = x[r].astype(f64) - mean32.astype(f64)
                grp[0] += d
                grp[1] += d * d
            out[g] = grp if w0 == g * ROWS else out[g] + grp
    return out


def ref_update(partials, rows, stats, table_mean32, eps, O):
    """partials [P, 2, O]; stats [1 + 2 O] = n | mean | M2 -> (stats', table' [2, O] float32): index-order sums, Chan's merge, the table."""
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


# ---- 1, 2: the apply stage -----------------------------------------------------------------------------------------------------------------------

SENTINEL = f32(-777.25)


def _run_apply(be, x, ld, table, table_ld, clip, with_partials, offset=0):
    """x [N, O] in rows of stride ld (pad columns = SENTINEL), `offset` floats into a 256-byte aligned buffer -> (y [N, ld], partials or None)."""
    N, O = x.shape
    host = np.full(offset + N * ld, SENTINEL, f32)
    rows = host[offset:].reshape(N, ld)
    rows[:, :O] = x
    tab = np.full((2, table_ld), 55.5, f32)
    tab[:, :O] = table
    dev, tdev = be.arr(host), be.arr(tab)
    G = be.lib.obs_norm_partials(N)
    assert G == -(-N // ROWS)
    part = be.full((G + 1, 2, O), np.nan, f64) if with_partials else None  # (one slab more than a launch may touch)
    be.lib.obs_norm_apply(N, O, be.ptr(dev) + 4 * offset, ld, be.ptr(tdev), table_ld, float(clip), be.ptr(part), be.stream)
    be.sync()
    out = be.host(dev)
    assert (out[:offset] == SENTINEL).all()
    p = be.host(part) if with_partials else None
    if p is not None:
        assert np.isnan(p[G]).all(), "a write beyond the launch's partials"
        p = p[:G]
    return out[offset:].reshape(N, ld).copy(), p


@pytest.mark.parametrize("N,O,ld,table_ld,offset", [(37, 225, 228, 228, 0), (300, 225, 228, 225, 0), (37, 7, 8, 8, 0), (300, 7, 8, 7, 0),
                                                     (37, 225, 228, 228, 1), (37, 7, 7, 7, 0), (37, 225, 230, 228, 0)])
def test_apply_is_the_float32_expression_bit_for_bit(be, N, O, ld, table_ld, offset):
    """The 16-byte form (aligned, ld a multiple of 4) and the one-column form (a base one float off, ld = 7, ld = 230) against NumPy float32."""
    rng = np.random.default_rng(N * 1000 + O + ld)
    x = (rng.standard_normal((N, O)) * rng.choice([0.1, 1.0, 30.0], O)[None, :]).astype(f32)
    table = np.stack([rng.standard_normal(O).astype(f32), rng.uniform(0.05, 3.0, O).astype(f32)])
    for clip in (0.0, 1.5):
        want = ref_apply(x, table, clip)
        if clip > 0:
            raw = ref_apply(x, table, 0.0)
            clamped = np.abs(raw) > clip
            assert clamped.any() and not clamped.all(), "the input must clamp some elements and leave others"
            assert (np.abs(want[clamped]) == f32(clip)).all() and np.array_equal(want[~clamped], raw[~clamped])
        y, part = _run_apply(be, x, ld, table, table_ld, clip, True, offset)
        assert np.array_equal(_bits(y[:, :O]), _bits(want)), f"clip {clip}"
        assert (y[:, O:] == SENTINEL).all(), "pad columns were written"
        y0, none = _run_apply(be, x, ld, table, table_ld, clip, False, offset)
        assert none is None and np.array_equal(_bits(y0), _bits(y)), "partial = NULL gives the same observations"
        # the partials come from the raw rows, whatever the clamp does (here on arbitrary inputs: the restatement's order)
        np.testing.assert_allclose(part, ref_partials(x, table[0]), rtol=1e-14, atol=0)


@pytest.mark.parametrize("N,O,ld", [(37, 225, 228), (300, 225, 228), (37, 7, 8), (40, 7, 7)])
def test_partials_are_exact_on_dyadic_inputs(be, N, O, ld):
    """Rows and means on the grid of multiples of 2^-6 within +-8: every d (a multiple of 2^-6 within +-16), every d^2 (of 2^-12, up to 256) and every
    sum over 128 rows is exact in float64 in any order, so the partials must EQUAL NumPy's sums over each workgroup's rows."""
    rng = np.random.default_rng(N + O)
    x = (rng.integers(-512, 513, (N, O)) / 64.0).astype(f32)
    table = np.stack([(rng.integers(-512, 513, O) / 64.0).astype(f32), np.full(O, 0.5, f32)])
    y, part = _run_apply(be, x, ld, table, O, 0.0, True)
    G = -(-N // ROWS)
    assert part.shape == (G, 2, O)
    d = x.astype(f64) - table[0].astype(f64)[None, :]
    for g in range(G):
        rows = d[g * ROWS:(g + 1) * ROWS]
        assert np.array_equal(part[g, 0], rows.sum(0)) and np.array_equal(part[g, 1], (rows * rows).sum(0)), g
    assert np.array_equal(part, ref_partials(x, table[0]))  # (and the restatement is those sums)
    assert np.array_equal(_bits(y[:, :O]), _bits(ref_apply(x, table, 0.0)))
    # the last workgroup holds N - 128 (G - 1) rows and nothing of a row beyond N: with one row more in the array, the same partials
    x1 = np.concatenate([x, np.full((1, O), 1000.0, f32)])
    host = np.full((N + 1) * ld, SENTINEL, f32)
    host.reshape(N + 1, ld)[:, :O] = x1
    dev, tdev, p2 = be.arr(host), be.arr(table), be.full((G, 2, O), np.nan, f64)
    be.lib.obs_norm_apply(N, O, be.ptr(dev), ld, be.ptr(tdev), O, 0.0, be.ptr(p2), be.stream)
    be.sync()
    assert np.array_equal(be.host(p2), part) and (be.host(dev).reshape(N + 1, ld)[N, :O] == 1000.0).all()


def test_apply_refuses_bad_arguments(be):
    f = be.lib._fn["mppo_obs_norm_apply"]
    obs, tab = be.zeros((4, 8)), be.zeros((2, 8))
    assert f(4, 7, be.ptr(obs), 8, be.ptr(tab), 8, -1.0, None, be.stream) == -1 and "negative" in be.lib.last_error()
    assert f(4, 7, be.ptr(obs), 8, be.ptr(tab), 8, float("nan"), None, be.stream) == -1
    assert f(4, 9, be.ptr(obs), 8, be.ptr(tab), 8, 0.0, None, be.stream) == -1 and "obs_ld" in be.lib.last_error()
    assert f(0, 7, be.ptr(obs), 8, be.ptr(tab), 8, 0.0, None, be.stream) == -1
    assert f(4, 7, None, 8, be.ptr(tab), 8, 0.0, None, be.stream) == -1
    assert be.lib.obs_norm_partials(0) == 0 and be.lib.obs_norm_partials(128) == 1 and be.lib.obs_norm_partials(129) == 2 and be.lib.obs_norm_partials(4096) == 32


# ---- 3: the update stage --------------------------------------------------------------------------------------------------------------------------


def _run_update(be, O, partials, rows, stats, table, table_ld, eps=EPS):
    tab = np.full((2, table_ld), 55.5, f32)
    tab[:, :O] = table
    sdev, tdev = be.arr(np.asarray(stats, f64)), be.arr(tab)
    pdev = be.arr(np.asarray(partials, f64)) if partials is not None else None
    be.lib.obs_norm_update(O, 0 if partials is None else len(partials), int(rows), be.ptr(pdev), be.ptr(sdev), float(eps), be.ptr(tdev), table_ld, be.stream)
    be.sync()
    return be.host(sdev).copy(), be.host(tdev).copy()


@pytest.mark.parametrize("O,table_ld,n0", [(225, 228, 0), (225, 228, 111), (7, 8, 0), (7, 7, 5000), (300, 300, 48)])
def test_update_merges_the_partials_like_the_restatement(be, O, table_ld, n0):
    """(n, mean, M2) given - n = 0 included - and 3 x 7 partials of 800 rows each: the statistics at rtol 1e-14 (a dozen float64 operations per column at
    2^-53 each), the table within one float32 ulp, the pad columns of the table 0 / 1.  O = 300: more columns than the workgroup has threads."""
    rng = np.random.default_rng(O + n0)
    scale = rng.choice([0.01, 1.0, 100.0], O)
    mean32 = (rng.standard_normal(O) * scale).astype(f32)
    xs = [(mean32[None, :] + rng.standard_normal((800, O)) * scale[None, :] + 0.3 * scale[None, :]).astype(f32) for _ in range(3)]
    partials = np.concatenate([ref_partials(x, mean32) for x in xs])
    assert partials.shape == (21, 2, O)
    if n0:
        stats = np.concatenate([[f64(n0)], rng.standard_normal(O) * scale, n0 * scale * scale * rng.uniform(0.5, 2.0, O)])
    else:
        stats = np.zeros(1 + 2 * O)
    got_stats, got_table = _run_update(be, O, partials, 2400, stats, np.stack([mean32, np.ones(O, f32)]), table_ld)
    want_stats, want_table = ref_update(partials, 2400, stats, mean32, EPS, O)
    assert got_stats[0] == n0 + 2400
    np.testing.assert_allclose(got_stats, want_stats, rtol=1e-14, atol=0)
    assert _ulps(got_table[:, :O], want_table) <= 1
    assert (got_table[0, O:] == 0).all() and (got_table[1, O:] == 1).all()
    # the same inputs, the same bytes
    again = _run_update(be, O, partials, 2400, stats, np.stack([mean32, np.ones(O, f32)]), table_ld)
    assert np.array_equal(_bits(again[0]), _bits(got_stats)) and np.array_equal(_bits(again[1]), _bits(got_table))


def test_update_without_rows_writes_the_table_of_the_statistics(be):
    O = 7
    # nothing counted, no partials: exactly the identity, whatever the table held
    stats, table = _run_update(be, O, None, 0, np.zeros(1 + 2 * O), np.full((2, O), 9.0, f32), 8)
    assert (stats == 0).all() and (table[0] == 0).all() and (table[1] == 1).all()
    # statistics given, no partials: they stay, the table is theirs
    st = np.concatenate([[10.0], np.arange(O) - 3.0, 10.0 * (1.0 + np.arange(O))])
    stats, table = _run_update(be, O, None, 0, st, np.zeros((2, O), f32), 8)
    assert np.array_equal(stats, st)
    want = ref_update(None, 0, st, None, EPS, O)[1]
    assert _ulps(table[:, :O], want) <= 1 and np.array_equal(table[0, :O], (np.arange(O) - 3.0).astype(f32))


def test_a_constant_column_gives_a_finite_table_and_output(be):
    """Column 2 of 7 holds 0.5 in every row: S1 = k / 2 and S2 = k / 4 exactly, M2 = 0, inv_std32 = float32(1 / sqrt(eps)), and the normalised column is 0."""
    N, O = 37, 7
    rng = np.random.default_rng(2)
    x = (rng.integers(-512, 513, (N, O)) / 64.0).astype(f32)
    x[:, 2] = 0.5
    ident = np.stack([np.zeros(O, f32), np.ones(O, f32)])
    _, part = _run_apply(be, x, 8, ident, 8, 0.0, True)
    stats, table = _run_update(be, O, part, N, np.zeros(1 + 2 * O), ident, 8)
    assert stats[0] == N and stats[1 + 2] == 0.5 and stats[1 + O + 2] == 0.0
    assert table[0, 2] == f32(0.5) and table[1, 2] == f32(1.0 / np.sqrt(f64(EPS))) and np.isfinite(table).all()
    y, _ = _run_apply(be, x, 8, table[:, :O], O, 10.0, False)
    assert np.isfinite(y[:, :O]).all() and (y[:, 2] == 0).all()
    f = be.lib._fn["mppo_obs_norm_update"]
    sdev, tdev = be.zeros((1 + 2 * O,), f64), be.zeros((2, 8))
    assert f(O, 0, 5, None, be.ptr(sdev), 1e-8, be.ptr(tdev), 8, be.stream) == -1 and "no partials" in be.lib.last_error()
    assert f(O, 0, 0, None, be.ptr(sdev), -1.0, be.ptr(tdev), 8, be.stream) == -1
    assert f(O, 0, 0, None, be.ptr(sdev), 1e-8, be.ptr(tdev), 6, be.stream) == -1


# ---- 4 - 7: the engine ----------------------------------------------------------------------------------------------------------------------------

NE, TE = 37, 3
ENGINE = [f"training.num_envs={NE}", f"training.num_steps={TE}", f"rl.num_env_steps={TE}", "training.num_minibatches=3", "training.update_epochs=1",
          "model.hidden_size=32", f"training.total_timesteps={NE * TE * 8}"]
NORM = ["training.normalize_observations=true", "training.obs_norm_clip=0"]
# a height window that ends episodes at every step (tests/test_evaluate.py, case "masked"): the reset-noise reinit then has rows to rewrite
FALLING = ["environment.reset_noise_scale=0.01", "reward.height_min_z=1.005", "reward.height_max_z=1.012"]


def _engine_stats_restated(obs_raw, O):
    """The statistics and table after ONE update from the identity: obs_raw [T, N, >= O] the raw rows of observation slots 1 .. T."""
    mean0 = np.zeros(O, f32)
    partials = np.concatenate([ref_partials(np.ascontiguousarray(o[:, :O]), mean0) for o in obs_raw])
    return ref_update(partials, obs_raw.shape[0] * obs_raw.shape[1], np.zeros(1 + 2 * O), mean0, EPS, O)


@pytest.mark.parametrize("extra", [[], FALLING], ids=["plain", "reset_noise"])
def test_first_rollout_is_the_plain_engines(be, extra):
    """The table is the identity until the first rollout's update has run: the normalising engine's first rollout leaves the plain engine's bytes, and its
    statistics are the restatement over observation slots 1 .. T (n = T N)."""
    plain = be.trainer(make_config(BASE, ENGINE + extra))
    norm = be.trainer(make_config(BASE, ENGINE + extra + NORM))
    for tr in (plain, norm):
        tr.reset()
    norm._sync()
    assert (norm._to_host(norm.region("obs_norm_stats")) == 0).all()
    t0 = norm._to_host(norm.region("obs_norm_table", (2, norm.OP)))
    assert (t0[0] == 0).all() and (t0[1] == 1).all()
    for tr in (plain, norm):
        tr.rollout()
        tr._sync()
    for name in ("obs", "action", "reward", "done", "adv", "value", "log_prob"):
        assert np.array_equal(_bits(plain._to_host(plain.region(name))), _bits(norm._to_host(norm.region(name)))), name
    if extra:
        assert plain._to_host(plain.region("done")).any(), "the window must end episodes: the reinit rewrote observation rows"
    O, OP = norm.O, norm.OP
    obs = plain._to_host(plain.region("obs", (TE + 1, NE, OP)))
    assert (obs[:, :, O:] == 0).all()
    want_stats, want_table = _engine_stats_restated(obs[1:], O)
    got = norm._to_host(norm.region("obs_norm_stats"))
    assert got[0] == TE * NE
    np.testing.assert_allclose(got, want_stats, rtol=1e-14, atol=0)
    table = norm._to_host(norm.region("obs_norm_table", (2, OP)))
    assert _ulps(table[:, :O], want_table) <= 1 and (table[0, O:] == 0).all() and (table[1, O:] == 1).all()
    assert norm.obs_norm()["count"] == TE * NE and np.array_equal(norm.obs_norm()["table"], table[:, :O])
    # the plain engine's regions are there and untouched (its arena starts zeroed)
    assert (plain._to_host(plain.region("obs_norm_stats")) == 0).all() and plain.obs_norm()["count"] == 0
    plain.close(); norm.close()


def _write_random(be, tr, rng):
    noise = rng.standard_normal((tr.T, tr.N, tr.A)).astype(f32)
    perms = np.stack([rng.permutation(tr.N * tr.T) for _ in range(tr.E)]).astype(np.int32)
    be.put(tr.region("noise", (tr.T, tr.N, tr.A)), noise)
    be.put(tr.region("perm", (tr.E, tr.N * tr.T)), perms)
    return noise


@pytest.mark.parametrize("extra", [[], ["training.obs_norm_clip=1.5"]], ids=["no_clip", "clip"])
def test_second_rollout_equals_the_composition_of_the_stages(be, extra):
    """Update 2's rollout written out with the ABI's own stages - mppo_policy_forward, mppo_env_step, mppo_obs_norm_apply per step, one
    mppo_obs_norm_update - from the engine's state, parameters, statistics and table after update 1: observations, actions, rewards, statistics and
    table bit for bit.  (Noise and permutations are written by the test: external_random.)"""
    cfg = make_config(BASE, ENGINE + NORM + extra)
    clip = float(cfg.training.obs_norm_clip)
    tr = be.trainer(cfg, external_random=True)
    tr.reset()
    rng = np.random.default_rng(11)
    _write_random(be, tr, rng)
    tr.update()
    tr._sync()
    N, Tn, O, OP, A = tr.N, tr.T, tr.O, tr.OP, tr.A
    host = lambda name, shape=None: np.array(tr._to_host(tr.region(name, shape)))
    stats1, table1 = host("obs_norm_stats"), host("obs_norm_table", (2, OP))
    assert stats1[0] == Tn * N and not (table1[0, :O] == 0).all() and not (table1[1, :O] == 1).all()
    state, rec, params = be.arr(host("state", (N, tr.dims.rec_dim))), be.arr(host("reset_rec")), be.arr(host("params"))
    obs = be.arr(host("obs", (Tn + 1, N, OP)))  # slot 0: update 1's last row, normalised with the identity
    met = {k: be.arr(host(k).astype(t)) for k, t in METRIC_TYPES.items()}
    noise = _write_random(be, tr, rng)
    tr.rollout()
    tr._sync()
    # ---- the replay
    lib, s = be.lib, be.stream
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    noise_d = be.arr(noise)
    act, logp, val, rew, done = be.zeros((Tn, N, A)), be.zeros((N,)), be.zeros((N,)), be.zeros((Tn, N)), be.zeros((Tn, N), np.uint8)
    wsb = lib.policy_ws_bytes(C.byref(tr.net), N)
    ws = be.zeros((wsb,), np.uint8)
    G = lib.obs_norm_partials(N)
    part, sdev, tdev = be.zeros((Tn, G, 2, O), f64), be.arr(stats1), be.arr(table1)
    rc = reward_cfg(cfg)
    row, arow, prow = N * OP * 4, N * A * 4, G * 2 * O * 8
    for t in range(Tn):
        lib.policy_forward(C.byref(tr.net), be.ptr(params), N, be.ptr(obs) + t * row, OP, be.ptr(noise_d) + t * arow, be.ptr(act) + t * arow, be.ptr(logp),
                           be.ptr(val), 0, be.ptr(ws), wsb, s)
        lib.env_step(tr._model, N, cfg.environment.n_frames, C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(act) + t * arow, A, be.ptr(obs) + (t + 1) * row, OP,
                     be.ptr(rew) + t * N * 4, be.ptr(done) + t * N, C.byref(M), s)
        lib.obs_norm_apply(N, O, be.ptr(obs) + (t + 1) * row, OP, be.ptr(tdev), OP, clip, be.ptr(part) + t * prow, s)
    lib.obs_norm_update(O, Tn * G, Tn * N, be.ptr(part), be.ptr(sdev), float(cfg.training.obs_norm_eps), be.ptr(tdev), OP, s)
    be.sync()
    for name, mine in (("obs", obs), ("action", act), ("reward", rew), ("obs_norm_partials", part), ("obs_norm_stats", sdev), ("obs_norm_table", tdev)):
        assert np.array_equal(_bits(host(name)).reshape(-1), _bits(be.host(mine)).reshape(-1)), name
    assert host("obs_norm_stats")[0] == 2 * Tn * N
    got = host("obs", (Tn + 1, N, OP))
    assert (got[:, :, O:] == 0).all(), "the pad columns of the stored observations stay zero"
    if clip > 0:
        assert np.abs(got[1:, :, :O]).max() == f32(clip), "the stored rows are clamped"
    assert not np.array_equal(got[1:], be.host(state)[None, :, :OP].repeat(Tn, 0)), "the stored rows are normalised, the state rows raw"
    tr.close()


def test_set_obs_norm_state_rules(be):
    cfg = make_config(BASE, ENGINE)
    f = be.lib._fn["mppo_engine_set_obs_norm"]
    tr = be.trainer(cfg)
    assert f(tr._engine, 1, -1.0, 1e-8) == -1 and "negative" in be.lib.last_error()  # MPPO_EINVAL
    assert f(tr._engine, 1, 10.0, -1e-8) == -1 and f(tr._engine, 1, float("nan"), 1e-8) == -1
    be.lib.engine_set_obs_norm(tr._engine, 1, 10.0, 1e-8)
    be.lib.engine_set_obs_norm(tr._engine, 0, 0.0, 0.0)
    tr.reset()
    assert f(tr._engine, 1, 10.0, 1e-8) == -4 and "mppo_engine_reset has run" in be.lib.last_error()  # MPPO_ESTATE
    tr.lib.engine_prepare(tr._engine, tr._stream_ptr)
    tr._sync()
    assert f(tr._engine, 1, 10.0, 1e-8) == -4 and "prepared" in be.lib.last_error()
    with pytest.raises(nat.NativeError):
        be.lib.engine_set_obs_norm(tr._engine, 0, 0.0, 0.0)
    tr.close()
    # several ranks: refused by the engine (the message names the ranks) and, before anything is created, by the Trainer
    even = [x for x in ENGINE if "num_envs" not in x and "minibatches" not in x] + ["training.num_envs=32", "training.num_minibatches=2"]
    two = be.trainer(make_config(BASE, even), world_size=2, rank=0)
    assert f(two._engine, 1, 10.0, 1e-8) == -1 and "world_size = 2 ranks" in be.lib.last_error()
    be.lib.engine_set_obs_norm(two._engine, 0, 10.0, 1e-8)  # (switching it off is nothing a rank count forbids)
    two.close()
    with pytest.raises(ValueError, match="2 ranks"):
        be.trainer(make_config(BASE, even + ["training.normalize_observations=true"]), world_size=2, rank=0)


def test_graph_replay_equals_eager_launches(be):
    """Three updates replayed from the captured graph and launched eagerly: the same parameters, statistics and table (on the emulator both are eager)."""
    cfg = make_config(BASE, ENGINE + NORM[:1] + FALLING[:1])
    out = {}
    for graph in (True, False):
        tr = be.trainer(cfg, use_graph=graph)
        tr.reset()
        for _ in range(3):
            tr.update()
        tr._sync()
        if be.name == "hip":
            assert tr.graph_active() == graph
        out[graph] = {n: np.array(tr._to_host(tr.region(n))) for n in ("params", "obs_norm_stats", "obs_norm_table", "obs")}
        assert out[graph]["obs_norm_stats"][0] == 3 * TE * NE
        tr.close()
    for n in out[True]:
        assert np.array_equal(_bits(out[True][n]), _bits(out[False][n])), n


# ---- 8: the evaluator -------------------------------------------------------------------------------------------------------------------------------

EV = dict(N=20, K=6, R=7, H=64, n_frames=5, noise=0.01, window=(1.005, 1.012), seed=5)
_EV = {}


def _ev_open(be):
    cm = load_model("synth_stompy_pro")
    h, dims, keep = be.model(cm)
    net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, EV["H"], 1, 0, 2)
    params = init_flat_params(3, dims.obs_dim, dims.nu, EV["H"])
    rc = reward_cfg(make_config(BASE, [f"reward.height_min_z={EV['window'][0]}", f"reward.height_max_z={EV['window'][1]}"]))
    e = nat.EvalCfg(N=EV["N"], K=EV["K"], n_frames=EV["n_frames"], deterministic=0, record_envs=EV["R"], reset_noise_scale=EV["noise"], seed=EV["seed"], reward=rc)
    return cm, h, dims, keep, net, params, rc, e


def _ev_table(O):
    rng = np.random.default_rng(8)
    return np.stack([(0.1 * rng.standard_normal(O)).astype(f32), rng.uniform(0.5, 2.0, O).astype(f32)])


def _ev_run(be, which, table=None, clip=0.0):
    """which: "plain" = mppo_evaluate, "norm" = mppo_evaluate_obs_norm (table None: the NULL table) -> (result bytes, trajectory)."""
    key = (be.name, which, None if table is None else table.tobytes(), clip)
    if key in _EV:
        return _EV[key]
    cm, h, dims, keep, net, params, rc, e = _ev_open(be)
    need = be.lib.eval_ws_bytes(h, C.byref(net), C.byref(e))
    ws, res = be.full((need,), 0xA5, np.uint8), be.full((C.sizeof(nat.EvalResultRaw) // 8,), -1, np.int64)
    traj = be.full((EV["K"] + 1, EV["R"], cm.nq + cm.nv + dims.nu + 2), np.nan)
    p_dev, t_dev = be.arr(params), None if table is None else be.arr(table)
    if which == "plain":
        be.lib.evaluate(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, be.ptr(res), be.ptr(traj), be.stream)
    else:
        be.lib.evaluate_obs_norm(h, C.byref(net), be.ptr(p_dev), C.byref(e), be.ptr(ws), need, be.ptr(t_dev), float(clip), be.ptr(res), be.ptr(traj), be.stream)
    be.sync()
    out = (be.host(res).tobytes(), be.host(traj).copy())
    be.lib.model_close(h)
    _EV[key] = out
    return out


def _ev_composed(be, table, clip):
    """The evaluation with a table written out with the library's own entry points -> trajectory rows and rewards."""
    cm, h, dims, keep, net, params, rc, e = _ev_open(be)
    N, K, R, OP, O, RD, A, nqv = EV["N"], EV["K"], EV["R"], dims.obs_pad, dims.obs_dim, dims.rec_dim, dims.nu, cm.nq + cm.nv
    lib, s = be.lib, be.stream
    state, rec, obs = be.zeros((N, RD)), be.zeros((RD,)), be.zeros((N, OP))
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    met = {k: be.full((N,), 3, t) for k, t in METRIC_TYPES.items()}
    M = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    p_dev, t_dev = be.arr(params), be.arr(table)
    act, logp, val, noise = be.zeros((N, A)), be.zeros((N,)), be.zeros((N,)), be.zeros((N, A))
    wsb = lib.policy_ws_bytes(C.byref(net), N)
    ws = be.zeros((wsb,), np.uint8)
    lib.env_reset(h, N, be.ptr(state), be.ptr(rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(M), s)
    lib.env_reinit(h, N, be.ptr(state), be.ptr(obs), OP, 0, EV["noise"], 0, EV["seed"], 0, 0, 0, 0, s)
    be.sync()
    frames = [np.concatenate([be.host(state)[:R, :nqv], np.zeros((R, A + 2), f32)], 1)]
    rewards = []
    for t in range(K):
        lib.normal_fill(EV["seed"], t, N * A, be.ptr(noise), s)
        lib.policy_forward(C.byref(net), be.ptr(p_dev), N, be.ptr(obs), OP, be.ptr(noise), be.ptr(act), be.ptr(logp), be.ptr(val), 0, be.ptr(ws), wsb, s)
        lib.env_step(h, N, EV["n_frames"], C.byref(rc), be.ptr(state), be.ptr(rec), be.ptr(act), A, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(M), s)
        lib.env_reinit(h, N, be.ptr(state), be.ptr(obs), OP, be.ptr(done), EV["noise"], 0, EV["seed"], 0, 0, 0, t + 1, s)
        lib.obs_norm_apply(N, O, be.ptr(obs), OP, be.ptr(t_dev), O, float(clip), 0, s)
        be.sync()
        frames.append(np.concatenate([be.host(state)[:R, :nqv], be.host(act)[:R], be.host(rew)[:R, None], (be.host(done)[:R, None] != 0).astype(f32)], 1))
        rewards.append(be.host(rew).copy())
    lib.model_close(h)
    return np.stack(frames).astype(f32), np.stack(rewards)


def test_evaluate_obs_norm_with_a_null_table_is_evaluate(be):
    plain, null = _ev_run(be, "plain"), _ev_run(be, "norm")
    assert plain[0] == null[0] and np.array_equal(_bits(plain[1]), _bits(null[1])) and not np.isnan(plain[1]).any()


@pytest.mark.parametrize("clip", [0.0, 0.75])
def test_evaluate_obs_norm_is_the_composition_with_the_apply_stage(be, clip):
    table = _ev_table(225)  # (synth_stompy_pro's observation)
    raw, traj = _ev_run(be, "norm", table, clip)
    frames, rewards = _ev_composed(be, table, clip)
    assert np.array_equal(_bits(traj), _bits(frames))
    r = nat.EvalResultRaw.from_buffer_copy(raw)
    assert r.steps == EV["N"] * EV["K"] and abs(r.reward_sum - rewards.astype(f64).sum()) <= 1e-12 * np.abs(rewards).astype(f64).sum()
    # the table is used: another policy input, another action (the policy's heads are small, not zero), another trajectory; the states before the
    # first forward are the same
    plain = _ev_run(be, "plain")[1]
    assert np.array_equal(_bits(traj[0]), _bits(plain[0])) and not np.array_equal(traj[2:], plain[2:])
    assert not np.array_equal(traj, _ev_run(be, "norm", table, 0.75 - clip)[1]), "the clamp changes what the policy reads"


# ---- 9 - 11: the Python layer ------------------------------------------------------------------------------------------------------------------------

SMALL = ["training.num_envs=8", "training.num_steps=2", "rl.num_env_steps=2", "training.num_minibatches=2", "training.update_epochs=1",
         "model.hidden_size=16", "training.total_timesteps=48"]
EVAL = dict(num_envs=8, num_steps=5, record_envs=4, deterministic=True)


def _kw(be):
    return dict(lib=be.lib, xp="numpy", use_graph=False) if be.name == "emu" else dict(device="cuda:0")


def _ev_kw(be):
    return dict(lib=be.lib, xp=be.xp)


def test_trainer_round_trip_through_the_model_file(be, tmp_path):
    path = str(tmp_path / "m.pkl")
    cfg = make_config(BASE, SMALL + ["training.normalize_observations=true", f"training.model_save_path={path}"])
    out = T.make_train(cfg, **_kw(be))(1337, log_every=1)
    assert len(out.metrics["total_loss"]) == 3 and np.isfinite(out.metrics["total_loss"]).all()
    tree = out.runner_state.train_state.params
    assert set(tree) == {"params", "obs_norm"} and set(tree["params"]) == {"MLP_0", "MLP_1", "log_std"}
    on = tree["obs_norm"]
    assert set(on) == {"mean", "inv_std", "clip", "count"} and on["count"] == 3 * 2 * 8 and on["clip"] == 10.0  # num_updates x T x N
    assert on["mean"].shape == (225,) and on["mean"].dtype == f32 and on["inv_std"].shape == (225,) and np.isfinite(on["inv_std"]).all()
    assert np.abs(on["mean"]).max() > 0.1 and not (on["inv_std"] == 1).all()
    T.save_model(tree, path)
    with open(path, "rb") as f:
        back = pickle.load(f)
    assert set(back) == {"params", "obs_norm"} and np.array_equal(back["obs_norm"]["mean"], on["mean"])
    flat = T.tree_to_flat(tree, 225, 10, 16)  # (ignores the sibling)
    a = evaluate(cfg, path, **_ev_kw(be), **EVAL)
    b = evaluate(cfg, flat, obs_norm=on, **_ev_kw(be), **EVAL)
    c = evaluate(cfg, flat, **_ev_kw(be), **EVAL)
    d = evaluate(cfg, tree, **_ev_kw(be), **EVAL)
    for k in ("qpos", "qvel", "action", "reward"):
        assert np.array_equal(_bits(a.trajectory[k]), _bits(b.trajectory[k])) and np.array_equal(_bits(a.trajectory[k]), _bits(d.trajectory[k])), k
    assert a.stats() == b.stats() or all(x == y or (x != x and y != y) for x, y in zip(a.stats().values(), b.stats().values()))
    assert not np.array_equal(a.trajectory["action"], c.trajectory["action"]), "without the table the policy reads other observations"
    with pytest.raises(ValueError, match="columns"):
        evaluate(cfg, flat, obs_norm={"mean": np.zeros(3, f32), "inv_std": np.ones(3, f32), "clip": 0.0}, **_ev_kw(be), **EVAL)
    # the last stored observation is the normalised row
    assert out.runner_state.last_obs.shape == (8, 225) and np.abs(out.runner_state.last_obs).max() <= 10.0
    # the option off: the tree is what it was
    off = T.make_train(make_config(BASE, SMALL), **_kw(be))(1337)
    assert set(off.runner_state.train_state.params) == {"params"}


def test_trainer_evaluate_uses_its_table(be):
    cfg = make_config(BASE, SMALL + ["training.normalize_observations=true"])
    tr = be.trainer(cfg)
    tr.reset()
    tr.update(); tr.update()
    on = tr.obs_norm()
    assert set(on) == {"count", "mean", "var", "table", "clip", "eps"} and on["count"] == 2 * 2 * 8 and on["eps"] == pytest.approx(1e-8)
    np.testing.assert_allclose(on["table"][1], 1.0 / np.sqrt(on["var"] + f64(f32(1e-8))), rtol=1e-6)
    tree = tr.params
    mine = tr.evaluate(**EVAL)
    tr.close()
    theirs = evaluate(cfg, tree, seed=cfg.training.seed, **_ev_kw(be), **EVAL)
    assert np.array_equal(_bits(mine.trajectory["action"]), _bits(theirs.trajectory["action"]))


def test_checkpoint_resume_is_bit_exact_and_refuses_the_other_setting(be, tmp_path):
    over = ["training.num_envs=24", "training.num_steps=3", "rl.num_env_steps=3", "training.num_minibatches=2", "training.update_epochs=1", "model.hidden_size=32",
            "training.total_timesteps=100000", "training.normalize_observations=true"]
    cfg = make_config(BASE, over)
    ck = str(tmp_path / "ck" / "state.npz")
    names = ("params", "adam_m", "obs_norm_stats", "obs_norm_table", "state")
    a = be.trainer(cfg)
    a.reset()
    a.update(); a.update()
    a.save_checkpoint(ck)
    a.update(); a.update()
    a._sync()
    want = {n: np.array(a._to_host(a.region(n))) for n in names}
    a.close()
    b = be.trainer(cfg)
    b.load_checkpoint(ck)
    assert b.updates_done == 2 and b.obs_norm()["count"] == 2 * 3 * 24
    b.update(); b.update()
    b._sync()
    for n in names:
        assert np.array_equal(_bits(b._to_host(b.region(n))), _bits(want[n])), n
    assert b.obs_norm()["count"] == 4 * 3 * 24
    b.close()
    c = be.trainer(make_config(BASE, over[:-1]))
    with pytest.raises(ValueError, match=r"normalize_observations=true.*normalize_observations=false"):
        c.load_checkpoint(ck)
    c.reset()
    c.update()
    ck2 = str(tmp_path / "ck" / "plain.npz")
    c.save_checkpoint(ck2)
    c.close()
    d = be.trainer(cfg)
    with pytest.raises(ValueError, match=r"normalize_observations=false.*normalize_observations=true"):
        d.load_checkpoint(ck2)
    d.close()


def test_config_keys():
    tr = make_config(BASE).training
    assert tr.normalize_observations is False and tr.obs_norm_clip == 10.0 and tr.obs_norm_eps == 1e-8
    tr = make_config(BASE, ["training.normalize_observations=true", "training.obs_norm_clip=0", "training.obs_norm_eps=1e-6"]).training
    assert tr.normalize_observations is True and tr.obs_norm_clip == 0.0 and tr.obs_norm_eps == pytest.approx(1e-6)
    assert make_config({**BASE, "training": {"normalize_observations": True, "obs_norm_clip": 5}}).training.obs_norm_clip == 5.0
    with pytest.raises(ValueError, match="obs_norm_clip"):
        make_config(BASE, ["training.obs_norm_clip=-1"])
    with pytest.raises(ValueError, match="obs_norm_eps"):
        make_config(BASE, ["training.obs_norm_eps=-1e-8"])
