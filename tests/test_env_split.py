"""The split form of the model-specialised environment step (minppo_amd/csrc/k_physics.hip, env_kernel's KMODE 5): an environment group - four
environments - run by a workgroup of TWO waves that divide the step's phases between them.  Which wave issues a phase is a
schedule, not arithmetic: the split form must equal the run-time-sized kernel and the unsplit specialised form bit for bit.

The library picks the form by the size of the launch (model_view.h split_launch): split while ceil(N / 4) <= 4 x compute units - at most one
wave per SIMD without it - and unsplit beyond.  The emulator stands for a device of four compute units (k_physics.hip kEmuCus), so launches of
up to 64 environments run split there, as launches of up to 16 x multi_processor_count do on the device.

Runs on the CPU emulator build (default) and on the MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from minppo_amd.model import load_model
from physics_harness import METRIC_TYPES

f32 = np.float32
MODEL = "synth_stompy_pro"  # the 16-dof stand-in: the one robot whose instantiation has a split step
EMU_CUS = 4


def _cus(be):
    if be.name == "emu":
        return EMU_CUS
    return be.torch.cuda.get_device_properties(be.dev).multi_processor_count


def _start(cm, dims, reset_state, N, seed):
    """Per-environment perturbed start records: the reset record with joint positions and all velocities moved, a different draw per environment."""
    rng = np.random.default_rng(seed)
    s = np.tile(reset_state, (N, 1)).astype(f32)
    s[:, 7:cm.nq] += (0.15 * rng.standard_normal((N, cm.nq - 7))).astype(f32)
    s[:, cm.nq:cm.nq + cm.nv] = (0.5 * rng.standard_normal((N, cm.nv))).astype(f32)
    return s


def _run(be, cm, N, steps, n_frames, start_seed, events=True, shared=None):
    """`steps` env steps of N environments from perturbed states; returns everything the step writes.  `shared`: only the first `shared` environments'
    states and actions are drawn (the same draws whatever N), the others repeat the first's."""
    h, dims, _keep = be.model(cm)
    flag = C.c_int32(-1)
    be.lib.model_is_specialized(h, C.byref(flag))
    OP, R, nu = dims.obs_pad, dims.rec_dim, cm.nu
    state, reset_rec, obs = be.zeros((N, R)), be.zeros((R,)), be.full((N, OP), np.nan)
    rew, done = be.zeros((N,)), be.zeros((N,), np.uint8)
    met = {k: be.zeros((N,), dt) for k, dt in METRIC_TYPES.items()}
    Ms = nat.EnvMetrics(**{k: be.ptr(v) for k, v in met.items()})
    be.lib.env_reset(h, N, be.ptr(state), be.ptr(reset_rec), be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), be.stream)
    be.sync()
    n_own = N if shared is None else shared
    s0 = _start(cm, dims, be.host(reset_rec), n_own, start_seed)
    if n_own < N:
        s0 = np.concatenate([s0, np.tile(s0[:1], (N - n_own, 1))])
    be.put(state, s0)
    rc = nat.RewardCfg(0.95, 2.0, 2.0, 0.2, 0.5, 0.1, 4.0, 1.0, 1.25)
    rng = np.random.default_rng(start_seed + 1)
    out = dict(done_steps=[], rew_steps=[], obs_steps=[])
    for t in range(steps):
        a = (0.7 * rng.standard_normal((n_own, nu))).astype(f32)
        if n_own < N:
            a = np.concatenate([a, np.tile(a[:1], (N - n_own, 1))])
        if events and t == 3:
            a[1, 2] = np.nan  # a NaN control (the robot's controls are range-limited: the clamp swallows it, the reward's control cost does not)
        if events and t == 6:
            s = be.host(state).copy()
            s[2, 2] = 0.3  # dropped below the height window: terminates, auto-reset
            be.put(state, s)
        if events and t == 9:
            s = be.host(state).copy()
            s[3, cm.nq] = np.nan  # a NaN velocity: cvel is NaN in the dynamics, the guard ends the episode and the reset record takes over
            be.put(state, s)
        da = be.arr(a)
        be.lib.env_step(h, N, n_frames, C.byref(rc), be.ptr(state), be.ptr(reset_rec), be.ptr(da), nu, be.ptr(obs), OP, be.ptr(rew), be.ptr(done), C.byref(Ms), be.stream)
        be.sync()
        out["done_steps"].append(be.host(done).copy())
        out["rew_steps"].append(be.host(rew).copy())
        out["obs_steps"].append(be.host(obs).copy())
    out.update(state=be.host(state).copy(), specialised=flag.value, **{k: be.host(v).copy() for k, v in met.items()})
    be.lib.model_close(h)
    return {k: np.asarray(v) for k, v in out.items()}


def _assert_bit_equal(a, b, what, rows=None):
    for k in a:
        if k == "specialised":
            continue
        x, y = a[k], b[k]
        if rows is not None:
            x, y = (x[:, :rows], y[:, :rows]) if k.endswith("_steps") else (x[:rows], y[:rows])
        neq = ~((x == y) | (np.isnan(x) & np.isnan(y))) if x.dtype.kind == "f" else x != y
        assert not neq.any(), (what, k, np.argwhere(neq)[:8].tolist())


@pytest.mark.parametrize("N,n_frames", [(4, 1), (5, 1), (24, 1), (24, 2), (64, 1)])
def test_split_step_equals_the_runtime_sized_kernel(be, monkeypatch, N, n_frames):
    """One group, a ragged group with surplus environments, several groups, the largest launch the emulator's selection rule still splits: twelve steps from
    per-environment perturbed states, one environment under a NaN control, one with a NaN velocity (the NaN guard: its flag crosses from the wave that runs
    the dynamics to the one that ends the step), one dropped out of the height window (auto-reset).  State records, observations, rewards, done flags and metrics, every step."""
    cm = load_model(MODEL)
    assert (N + 3) // 4 <= 4 * _cus(be)  # (split by the rule)
    monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
    split = _run(be, cm, N, 12, n_frames, 40 + N)
    monkeypatch.setenv("MPPO_ENV_GENERIC", "1")
    generic = _run(be, cm, N, 12, n_frames, 40 + N)
    monkeypatch.delenv("MPPO_ENV_GENERIC", raising=False)
    assert split["specialised"] == 1 and generic["specialised"] == 0
    # the events happened: the NaN control reached the reward, the drop and the NaN velocity each ended an episode, and the reset record took over
    assert np.isnan(generic["rew_steps"][3][1]) and generic["done_steps"][6][2] == 1 and generic["done_steps"][9][3] == 1
    assert np.isfinite(generic["state"]).all()
    _assert_bit_equal(split, generic, f"N={N} frames={n_frames}")


def test_split_step_equals_the_unsplit_specialised_step(be):
    """The largest launch that runs split (four environment groups per compute unit: one wave per SIMD unsplit) and one group more (unsplit by the rule),
    the shared environments from identical states under identical controls: bit-equal after three steps."""
    cm = load_model(MODEL)
    n_split = 16 * _cus(be)
    a = _run(be, cm, n_split, 3, 1, 7, events=False, shared=n_split)
    b = _run(be, cm, n_split + 4, 3, 1, 7, events=False, shared=n_split)
    assert a["specialised"] == 1 and b["specialised"] == 1
    _assert_bit_equal(a, b, "split vs unsplit", rows=n_split)
