"""Wide observations on the depth-generic row pass (csrc/k_deep.hip): the streamed first layer (96-column slabs through a two-slab LDS ring) and two hidden layers
where the fused kernels refuse, against the float64 oracle and, on dyadic operands, bit for bit; on the emulator and (-m gpu) on the MI355X."""
import ctypes as C

import numpy as np
import pytest

from minppo_amd import _native as nat
from oracle import ppo_oracle as po
from test_deep_rowpass import _paths
from test_exact_products import _forward_exact, _GradCase
from test_kernels_ppo import _net, _params

# (layers, O, A, H, B, mb, tanh, ref).  ref: the LAYER-WISE kernels' error against the same oracle on the same inputs, measured (the larger of emulator and MI355X) at the parent
# commit - the last case, beyond the 2^20 parameters its gradient took, on this tree's layer-wise path: (mean, value, action, log_prob, loss / its largest term, grad / a tensor's largest entry)
CASES = [(4, 1221, 3, 256, 40, 22, 1, (1.40e-6, 3.86e-6, 1.43e-6, 1.28e-6, 8.89e-8, 3.97e-6)),    # streamed at the deepest LDS budget: KP = 1248 > 1216; O = 38 . 32 + 5; partial last tile
         (3, 2531, 17, 32, 90, 70, 0, (3.61e-6, 3.15e-6, 3.63e-6, 3.25e-6, 4.49e-8, 1.58e-5)),   # streamed in both roles, one wave: 27 slabs, the last of two stages; OT = 2; ReLU; idx a subset
         (1, 2400, 3, 64, 32, 32, 1, (5.70e-7, 1.87e-6, 5.60e-7, 8.90e-7, 2.32e-8, 5.10e-6)),    # streamed, whole slabs: O = OP = KP = 25 . 96, no K tail; two waves; no backward product
         (2, 800, 6, 256, 48, 48, 1, (7.61e-7, 1.79e-6, 7.60e-7, 1.56e-6, 2.48e-8, 2.49e-6)),    # two layers beyond the weight-gradient tile table (O > 736), x tile resident
         (2, 1763, 10, 256, 48, 40, 1, (1.83e-6, 2.88e-6, 1.83e-6, 1.34e-6, 1.15e-8, 3.62e-6)),  # two layers, streamed: KP = 1792 > 1728, the last slab of two stages
         (3, 1575, 28, 256, 32, 24, 1, (1.37e-6, 4.64e-6, 1.43e-6, 5.78e-6, 3.06e-8, 4.44e-6))]  # the 93-body robot's network, streamed: 1.08 M parameters, beyond 2^20


@pytest.mark.parametrize("layers,O,A,H,B,mb,tanh,ref", CASES)
def test_wide_rowpass_matches_the_oracle(be, layers, O, A, H, B, mb, tanh, ref):
    rng, f32, f64, nan = np.random.default_rng(11), np.float32, np.float64, np.nan
    net, OP, AP = _net(O, A, H, tanh, 0, layers), (O + 3) // 4 * 4, (A + 3) // 4 * 4
    flat, n64 = _params(rng, O, A, H, layers=layers)
    bobs = np.zeros((B, OP), f32); bobs[:, :O] = rng.standard_normal((B, O))
    noise = rng.standard_normal((B, A)).astype(f32)
    d_flat, d_obs, d_noise, ws = be.arr(flat), be.arr(bobs), be.arr(noise), be.full((be.lib.policy_ws_bytes(C.byref(net), B) // 4 + 4,), nan)
    act, logp, value, value2, mean = be.full((B, A), nan), be.full((B,), nan), be.full((B,), nan), be.full((B,), nan), be.full((B, AP), nan)
    fwd = lambda *outs: be.lib.policy_forward(C.byref(net), be.ptr(d_flat), B, be.ptr(d_obs), OP, *outs, be.ptr(ws), be.lib.policy_ws_bytes(C.byref(net), B), be.stream)
    fwd(be.ptr(d_noise), be.ptr(act), be.ptr(logp), be.ptr(value), be.ptr(mean))  # the sample form
    fwd(None, None, None, be.ptr(value2), None)                                   # the value-only form (noise = NULL: the bootstrap call)
    m64, ls64, v64 = po.actor_critic_forward(n64, bobs[:, :O].astype(f64), bool(tanh))
    a64 = po.mvn_sample(m64, ls64, noise.astype(f64))
    err = [np.abs(got - w).max() for got, w in ((be.host(mean)[:, :A], m64), (np.stack([be.host(value), be.host(value2)]), v64), (be.host(act), a64),
                                                (be.host(logp), po.mvn_log_prob(a64, m64, ls64)))]
    b = dict(act=rng.standard_normal((B, A)), val=v64 + 0.3 * rng.standard_normal(B))  # ---- mppo_minibatch_grad
    b.update(lp=po.mvn_log_prob(b["act"].astype(f32).astype(f64), m64, ls64) + 0.3 * rng.standard_normal(B), adv=rng.standard_normal(B) * 3 + 1, tgt=rng.standard_normal(B))
    b, idx = {k: v.astype(f32) for k, v in b.items()}, rng.permutation(B)[:mb].astype(np.int32)
    g = b["adv"][idx].astype(f64)
    d = {k: be.arr(v) for k, v in dict(b, idx=idx, st=np.array([g.mean(), 1 / (g.std() + 1e-8)], f32)).items()}
    batch = nat.Batch(be.ptr(d_obs), OP, be.ptr(d["act"]), A, be.ptr(d["val"]), be.ptr(d["lp"]), be.ptr(d["adv"]), be.ptr(d["tgt"]))
    grad, loss4, gwsb, st = be.full((flat.size,), nan), be.full((4,), nan), be.lib.grad_ws_bytes(C.byref(net), mb), be.host(d["st"])
    gws = be.full((gwsb // 4 + 4,), nan)
    be.lib.minibatch_grad(C.byref(net), be.ptr(d_flat), C.byref(batch), be.ptr(d["idx"]), mb, be.ptr(d["st"]), 1.0 / mb, C.byref(nat.LossCfg(0.2, 0.5, 0.01)), be.ptr(grad),
                          be.ptr(loss4), be.ptr(gws), gwsb, be.stream)
    lo, gr = po.loss_and_grad(n64, *[x[idx].astype(f64) for x in (bobs[:, :O], b["act"], b["val"], b["lp"])], g, b["tgt"][idx].astype(f64), 0.2, 0.5, 0.01, bool(tanh), adv_mean=float(st[0]), adv_std=1.0 / float(st[1]) - 1e-8)
    got, g64 = be.host(grad), po.named_to_flat(gr, O, A, H)
    err += [np.abs(be.host(loss4) - lo).max() / np.abs(lo).max(), max(np.abs(got[o:o + int(np.prod(s))] - g64[o:o + int(np.prod(s))]).max() / np.abs(g64[o:o + int(np.prod(s))]).max() for o, s in po.param_slices(O, A, H, layers).values())]
    assert _paths(be, net, d_obs, OP) in ([(2, 2), (2, 1)] if layers == 2 else [(2, 2)])  # (two layers: the fused rollout kernel has no tile table and keeps them up to its own LDS limit)
    assert all(e <= 2 * r for e, r in zip(err, ref)), (err, ref)  # twice the layer-wise error: exact float32 products on both sides, another order of the sums (a NaN left fails)


@pytest.mark.parametrize("layers,O,A,H,grad,paths", [(3, 1477, 3, 256, True, (2, 2)), (3, 2307, 3, 256, False, (2, 2)), (2, 800, 6, 256, True, (2, 1))])
def test_wide_rowpass_exact(be, layers, O, A, H, grad, paths):
    """Dyadic operands, every partial sum exact: float64 bit for bit.  Streamed row pass (KP = 1504 > 1472) | streamed rollout (KP = 2336 > 2272), forward only | two layers, unfused."""
    assert _paths(be, _net(O, A, H, 0, 0, layers), be.zeros((4, (O + 3) // 4 * 4)), (O + 3) // 4 * 4) == paths
    _forward_exact(be, O, A, H, 21, 0, layers)
    grad and _GradCase(be, O, A, H, 32, 0, layers).run()
