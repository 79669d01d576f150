"""Wide observations in bf16: the bf16 row pass with a resident x tile (csrc/k_deep_bf16.hip: wide_bf16_kernel) where the fused kernels refuse a two-layer bf16 network,
against the oracle with the same operand rounding (oracle/ppo_oracle.py, bf16=True); on the emulator and (-m gpu) on the MI355X."""
import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from oracle import ppo_oracle as po
from test_deep_rowpass import _paths
from test_engine import _cfg
from test_kernels_ppo import _net, _params

f32, f64 = np.float32, np.float64
# (O, A, H, B, mb, tanh, rollout path).  The smallest H at which the weight-gradient tile table (512 tiles) still refuses the width; tolerances: those of
# test_kernels_ppo.py::test_bf16_mfma_path, unchanged.  Measured on the CPU at these shapes, the same-rounding oracle evaluated in float32 against itself in float64 (worst
# tensor, relative to its largest entry | loss): 9.2e-4 | 1.2e-7 at K = 800, 3.2e-5 | 6.6e-8 at K = 1575, 1.3e-6 | 4.3e-8 at K = 2403 - with 4x for the order of the sums
# 3.7e-3, inside the 5e-3 per tensor and 2e-3 of the loss that the narrow shapes are held to (what they bound: values on the other side of a bf16 rounding boundary)
CASES = [(800, 6, 256, 48, 48, 1, 1),    # just past the fused kernels' reach (O > 736), whole row tiles, eight waves
         (1575, 28, 160, 32, 24, 1, 1),  # the 93-body robot's width, O = 49 . 32 + 7; two output tiles; a last tile of 8 rows; idx a subset; five waves, 20 threads per x row
         (2403, 3, 64, 22, 22, 0, 2)]    # beyond the fused ROLLOUT kernel's LDS as well: both roles here; ReLU actor; two waves; a last tile of 6 rows


@pytest.mark.parametrize("O,A,H,B,mb,tanh,rollout", CASES)
def test_wide_bf16_rowpass_matches_the_bf16_oracle(be, O, A, H, B, mb, tanh, rollout):
    rng, nan = np.random.default_rng(5), np.nan
    net, OP, AP = _net(O, A, H, tanh, bf16=1), (O + 3) // 4 * 4, (A + 3) // 4 * 4
    flat, n64 = _params(rng, O, A, H)
    bobs = np.zeros((B, OP), f32); bobs[:, :O] = rng.standard_normal((B, O))
    noise = rng.standard_normal((B, A)).astype(f32)
    d_flat, d_obs, d_noise = be.arr(flat), be.arr(bobs), be.arr(noise)
    assert _paths(be, _net(O, A, H, tanh, 0), d_obs, OP)[0] == 2 and _paths(be, net, d_obs, OP) == (2, rollout)
    # ---- rollout forward
    wsb = be.lib.policy_ws_bytes(C.byref(net), B)
    ws, act, logp, value, mean = be.full((wsb // 4 + 4,), nan), be.full((B, A), nan), be.full((B,), nan), be.full((B,), nan), be.full((B, AP), nan)
    be.lib.policy_forward(C.byref(net), be.ptr(d_flat), B, be.ptr(d_obs), OP, be.ptr(d_noise), be.ptr(act), be.ptr(logp), be.ptr(value), be.ptr(mean), be.ptr(ws), wsb, be.stream)
    x64 = bobs[:, :O].astype(f64)
    mb16, ls, vb16, (ha, hc) = po.actor_critic_forward(n64, x64, bool(tanh), keep=True, bf16=True)
    mex, _, vex = po.actor_critic_forward(n64, x64, bool(tanh))
    np.testing.assert_allclose(be.host(mean)[:, :A], mb16, atol=2e-3 * np.abs(mex).max() + 1e-5)
    np.testing.assert_allclose(be.host(value), vb16, atol=2e-3 * np.abs(vex).max() + 1e-5)
    assert np.abs(be.host(mean)[:, :A] - mex).max() > 1e-6  # it really is a different arithmetic
    np.testing.assert_allclose(be.host(logp), po.mvn_log_prob(be.host(act).astype(f64), be.host(mean)[:, :A].astype(f64), ls), atol=1e-4)
    # ---- mppo_minibatch_grad: the rollout's own actions and log-probs as the old policy's, so that every ratio is 1
    b = dict(act=be.host(act), lp=be.host(logp), val=(vex + 0.3 * rng.standard_normal(B)).astype(f32), adv=(rng.standard_normal(B) * 3 + 1).astype(f32), tgt=rng.standard_normal(B).astype(f32))
    idx = rng.permutation(B)[:mb].astype(np.int32)
    st = np.array([0.3, 0.7], f32)
    d = {k: be.arr(v) for k, v in dict(b, idx=idx, st=st).items()}
    batch = nat.Batch(be.ptr(d_obs), OP, be.ptr(d["act"]), A, be.ptr(d["val"]), be.ptr(d["lp"]), be.ptr(d["adv"]), be.ptr(d["tgt"]))
    gwsb = be.lib.grad_ws_bytes(C.byref(net), mb)
    grad, loss4, gws = be.full((flat.size,), nan), be.full((4,), nan), be.full((gwsb // 4 + 4,), nan)
    be.lib.minibatch_grad(C.byref(net), be.ptr(d_flat), C.byref(batch), be.ptr(d["idx"]), mb, be.ptr(d["st"]), 1.0 / mb, C.byref(nat.LossCfg(0.2, 0.5, 0.0)), be.ptr(grad),
                          be.ptr(loss4), be.ptr(gws), gwsb, be.stream)
    g = b["adv"][idx].astype(f64)
    args64 = (*[v[idx].astype(f64) for v in (bobs[:, :O], b["act"], b["val"], b["lp"])], g, b["tgt"][idx].astype(f64), 0.2, 0.5, 0.0, bool(tanh))
    kw = dict(adv_mean=float(st[0]), adv_std=1.0 / float(st[1]) - 1e-8)
    lo_b, gr_b = po.loss_and_grad(n64, *args64, bf16=True, **kw)
    lo_x, gr_x = po.loss_and_grad(n64, *args64, **kw)
    got, gb, gx, l4 = be.host(grad), po.named_to_flat(gr_b, O, A, H), po.named_to_flat(gr_x, O, A, H), be.host(loss4)
    np.testing.assert_allclose(l4, lo_b, rtol=2e-3, atol=1e-5)  # same rounding: only boundary flips remain
    np.testing.assert_allclose(l4[2], -np.mean((g - st[0]) * st[1]), rtol=2e-3, atol=1e-5)  # the training pass reproduces the rollout's log_prob: the actor loss at ratio 1
    cos = lambda a, c: float(a @ c / (np.linalg.norm(a) * np.linalg.norm(c)))
    assert cos(got, gb) > 0.99999, cos(got, gb)
    assert cos(got, gx) > min(0.999, cos(gb, gx) - 1e-4), (cos(got, gx), cos(gb, gx))  # as close to exact arithmetic as the bf16 oracle is
    sl = po.param_slices(O, A, H)
    for k, (o, s) in sl.items():
        sz = int(np.prod(s))
        np.testing.assert_allclose(got[o:o + sz], gb[o:o + sz], rtol=0, atol=5e-3 * np.abs(gb[o:o + sz]).max() + 1e-7, err_msg=k)
    # ---- what the row pass left in the workspace (ppo_layout.h carve_grad): activations as the oracle's; dZ rounded to bf16, its column sums the bias gradients
    w, mbp = be.host(gws), (mb + 15) // 16 * 16
    nh, at = mbp * H, lambda off: w[off:off + mb * H].reshape(mb, H)
    dz0 = 4 * nh + mbp * AP + mbp + mbp * (AP + 4)
    for off, want in zip((0, nh, 2 * nh, 3 * nh), (ha[0], ha[1], hc[0], hc[1])):
        np.testing.assert_allclose(at(off), want[idx], atol=2e-3 * np.abs(want).max() + 1e-5)
    for off, name in zip((dz0, dz0 + nh, dz0 + 2 * nh, dz0 + 3 * nh), ("a_b2", "c_b2", "a_b1", "c_b1")):
        dz, want = at(off), gb[sl[name][0]:sl[name][0] + H]
        assert not (dz.view(np.uint32) & 0xFFFF).any(), name
        np.testing.assert_allclose(dz.astype(f64).sum(0), want, rtol=0, atol=5e-3 * np.abs(want).max() + 1e-7, err_msg=name)


def test_engine_trains_the_wide_robot_in_bf16(be):
    """Two updates of a small engine on the 93-body stand-in (O = 1575) with training.mlp_dtype = bf16: the rollout on the fused kernel, the optimizer steps on the bf16 row
    pass and the layer-wise bf16 weight gradients; the first update's PPO half against the same-rounding oracle as tests/test_engine.py's bf16 case does it."""
    from oracle.env_oracle import default_hp
    emu = be.name == "emu"
    cfg = _cfg("environment.model=synth_stompy_frames", "training.mlp_dtype=bf16", "model.hidden_size=160", f"training.num_envs={8 if emu else 64}", "training.num_steps=4",
               "rl.num_env_steps=4", "training.num_minibatches=2", "training.update_epochs=2", "training.total_timesteps=100000000")
    tr = be.trainer(cfg, external_random=True, use_graph=False)
    tr.reset()
    N, T, A, H, O, E, M = tr.N, tr.T, tr.A, tr.H, tr.O, tr.E, tr.M
    assert O == 1575 and _paths(be, tr.net, tr.region("obs"), tr.net.OP) == (2, 1)
    rng = np.random.default_rng(0)
    p = tr.params_flat().astype(f64)
    be.put(tr.region("noise", (T, N, A)), rng.standard_normal((T, N, A)).astype(f32))
    perms = np.stack([rng.permutation(N * T) for _ in range(E)]).astype(np.int32)
    be.put(tr.region("perm", (E, N * T)), perms)
    tr.rollout()
    tr._sync()
    tj = {k: be.host(v).copy() for k, v in tr.traj().items()}
    tr.learn()
    traj = dict(obs=tj["obs"][:T, :, :O].astype(f64), action=tj["action"].astype(f64), value=tj["value"].astype(f64), log_prob=tj["log_prob"].astype(f64))
    p_new, _, losses = po.update_epochs_on_batch(p, po.OptState(np.zeros_like(p), np.zeros_like(p), 0), traj, tj["adv"].astype(f64), tj["target"].astype(f64), perms, O=O, A=A, H=H, num_minibatches=M, hp=dict(default_hp(cfg), mlp_bf16=True))
    got, step = tr.params_flat(), np.abs(p_new - p).max()
    assert np.abs(got - p_new).max() < 0.15 * step, (np.abs(got - p_new).max(), step)
    np.testing.assert_allclose(tr.losses()[..., :2], losses[..., :2], rtol=5e-3, atol=5e-4)
    be.put(tr.region("noise", (T, N, A)), rng.standard_normal((T, N, A)).astype(f32))
    tr.update()
    after = tr.params_flat()
    assert np.isfinite(after).all() and np.abs(after - got).max() > 0 and int(be.host(tr.region("count"))[0]) == 2 * E * M
    tr.close()
