"""The depth-generic row pass (csrc/k_deep.hip: deep_mlp_kernel) for networks of 1, 3 and 4 hidden layers against the float64 oracle:
`mppo_policy_forward` (sample form and value-only form) and `mppo_minibatch_grad`, on the emulator and (-m gpu) on the MI355X."""
import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from oracle import ppo_oracle as po
from test_kernels_ppo import _net, _params

f32 = np.float32


def _paths(be, net, obs, OP):
    rowpass, rollout = C.c_int32(-1), C.c_int32(-1)
    be.lib.network_path(C.byref(net), be.ptr(obs), OP, C.byref(rowpass), C.byref(rollout))
    return rowpass.value, rollout.value


# (layers, O, A, H, B, mb, tanh): the smallest shapes at which this kernel can go wrong
@pytest.mark.parametrize("layers,O,A,H,B,mb,tanh", [
    (1, 37, 3, 32, 40, 22, 1),     # one wave; no backward product at all; partial last tile (22 = 16 + 6); K tail: 37 -> OP = 40, KP = 64
    (3, 37, 3, 64, 90, 70, 0),     # ReLU actor; idx a strict subset of the batch
    (3, 35, 17, 96, 48, 48, 1),    # OT = 2 (A > 16); three waves; O = 32 + 3; whole tiles only
    (4, 24, 2, 256, 32, 20, 1),    # eight waves at the deepest depth: the largest LDS budget; O below one k stage
    (3, 225, 10, 256, 64, 64, 1),  # the production geometry at three layers
])
def test_deep_rowpass_matches_the_oracle(be, layers, O, A, H, B, mb, tanh):
    rng = np.random.default_rng(11)
    net = _net(O, A, H, tanh, 0, layers)
    OP, AP = net.OP, (A + 3) // 4 * 4
    flat, n64 = _params(rng, O, A, H, layers=layers)
    bobs = np.zeros((B, OP), f32); bobs[:, :O] = rng.standard_normal((B, O))
    x64 = bobs[:, :O].astype(np.float64)
    d_flat, d_obs = be.arr(flat), be.arr(bobs)
    assert _paths(be, net, d_obs, OP) == (2, 2)
    # ---- mppo_policy_forward, sample form
    noise = rng.standard_normal((B, A)).astype(f32)
    d_noise = be.arr(noise)
    act, logp, value, mean = be.zeros((B, A)), be.zeros((B,)), be.zeros((B,)), be.zeros((B, AP))
    wsb = be.lib.policy_ws_bytes(C.byref(net), B)
    ws = be.full((wsb // 4 + 4,), np.nan)
    be.lib.policy_forward(C.byref(net), be.ptr(d_flat), B, be.ptr(d_obs), OP, be.ptr(d_noise), be.ptr(act), be.ptr(logp), be.ptr(value), be.ptr(mean),
                          be.ptr(ws), wsb, be.stream)
    m64, ls64, v64 = po.actor_critic_forward(n64, x64, bool(tanh))
    a64 = po.mvn_sample(m64, ls64, noise.astype(np.float64))
    np.testing.assert_allclose(be.host(mean)[:, :A], m64, atol=2e-5)
    np.testing.assert_allclose(be.host(value), v64, atol=2e-5)
    np.testing.assert_allclose(be.host(act), a64, atol=2e-5)
    np.testing.assert_allclose(be.host(logp), po.mvn_log_prob(a64, m64, ls64), atol=5e-5)
    # ---- value-only form (noise = NULL: the bootstrap call)
    value2 = be.full((B,), np.nan)
    be.lib.policy_forward(C.byref(net), be.ptr(d_flat), B, be.ptr(d_obs), OP, None, None, None, be.ptr(value2), None, be.ptr(ws), wsb, be.stream)
    np.testing.assert_allclose(be.host(value2), v64, atol=2e-5)
    # ---- mppo_minibatch_grad
    bact = rng.standard_normal((B, A)).astype(f32)
    bval = (v64 + 0.3 * rng.standard_normal(B)).astype(f32)
    blp = (po.mvn_log_prob(bact.astype(np.float64), m64, ls64) + 0.3 * rng.standard_normal(B)).astype(f32)
    badv = (rng.standard_normal(B) * 3 + 1).astype(f32)
    btgt = rng.standard_normal(B).astype(f32)
    idx = rng.permutation(B)[:mb].astype(np.int32)
    d = {k: be.arr(v) for k, v in dict(act=bact, val=bval, lp=blp, adv=badv, tgt=btgt, idx=idx).items()}
    g = badv[idx].astype(np.float64)
    stats = be.arr(np.array([g.mean(), 1 / (g.std() + 1e-8)], f32))
    batch = nat.Batch(be.ptr(d_obs), OP, be.ptr(d["act"]), A, be.ptr(d["val"]), be.ptr(d["lp"]), be.ptr(d["adv"]), be.ptr(d["tgt"]))
    lc = nat.LossCfg(0.2, 0.5, 0.01)
    grad, loss4 = be.full((flat.size,), np.nan), be.zeros((4,))
    gwsb = be.lib.grad_ws_bytes(C.byref(net), mb)
    gws = be.full((gwsb // 4 + 4,), np.nan)
    be.lib.minibatch_grad(C.byref(net), be.ptr(d_flat), C.byref(batch), be.ptr(d["idx"]), mb, be.ptr(stats), 1.0 / mb, C.byref(lc), be.ptr(grad),
                          be.ptr(loss4), be.ptr(gws), gwsb, be.stream)
    lo, gr = po.loss_and_grad(n64, x64[idx], bact[idx].astype(np.float64), bval[idx].astype(np.float64), blp[idx].astype(np.float64), g,
                              btgt[idx].astype(np.float64), 0.2, 0.5, 0.01, bool(tanh), adv_mean=float(be.host(stats)[0]),
                              adv_std=1.0 / float(be.host(stats)[1]) - 1e-8)
    np.testing.assert_allclose(be.host(loss4), lo, rtol=1e-5, atol=1e-6)
    got, g64 = be.host(grad), po.named_to_flat(gr, O, A, H)
    assert not np.isnan(got).any() and got.size == g64.size
    for k, (o, s) in po.param_slices(O, A, H, layers).items():
        sz = int(np.prod(s))
        np.testing.assert_allclose(got[o:o + sz], g64[o:o + sz], rtol=0, atol=1e-4 * np.abs(g64[o:o + sz]).max() + 1e-7, err_msg=k)


def test_network_path_query(be):
    obs = be.zeros((4, 40))
    assert _paths(be, _net(37, 3, 64, 1, 0, 2), obs, 40) == (1, 1)  # two layers: the fused kernels
    assert _paths(be, _net(37, 3, 512, 1, 0, 3), obs, 40) == (0, 0)  # H > 256 and H % 32 != 0 stay layer-wise
    assert _paths(be, _net(37, 3, 48, 1, 0, 3), obs, 40) == (0, 0)
    with pytest.raises(nat.NativeError):
        _paths(be, _net(37, 3, 64, 1, 0, 5), obs, 40)
