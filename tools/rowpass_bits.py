"""tools/rowpass_bits.py <library> [--no-engine] - sha256 of everything the row-pass kernels of csrc/k_fused.hip write, for a given build of
the library: run it with two builds (e.g. the parent commit's and this tree's) and diff the outputs; equal lines = equal bits.  A library
whose file name contains "emu" is the CPU emulator build (tests/emu/libminppo_emu.so, NumPy arrays as device memory); any other is
loaded as the HIP library on cuda:0.  profiles/rowpass_split_bits.txt holds its output for the row-pass split.

Cases (B = 96 samples, fixed seeds):
  training  (O, A, H, mb) = (37, 5, 64, 42), (37, 5, 64, 48), (37, 20, 64, 48) - one and two 16-wide output tiles, a minibatch that is no
            multiple of 16 - float and bf16, tanh and relu, through mppo_minibatch_grad, mppo_minibatch_grad_shadow and mppo_gather_rows +
            mppo_minibatch_grad_pre twice (with idx_next at parity 0, without at parity 1; bf16 runs bf16_rowpass_kernel there).  Hashed: the whole
            NaN-prefilled gradient workspace, grad, loss4.
  32 rows   the float pre-gathered path at the smallest shape that selects 32-row tiles (asserted through mppo_minibatch_rows_per_workgroup):
            emulator mb = 64 at H = 64; GPU O = 37, A = 5 / 20, H = 256, mb = 2080 (130 sixteen-row tiles: the first even count above half of 256 CUs)
  rollout   mppo_policy_forward at n = 33 for the same geometries and dtypes, with noise + value and value-only (the C ABI requires `value`, so the
            actor-alone launch is not reachable through it); hashed: action, log_prob, value, mean_out
  wide      O = 415 and O = 447, A = 20, H = 256, mb = 48 / n = 33: 64 320 and 66 368 bytes of LDS - just under and above the 64 KB from which a launch
            needs the dynamic-LDS attribute - for both roles
  engine    (unless --no-engine) a 64-environment rollout, an update and a second rollout of a bf16 and a float network through the engine: the
            only caller that hands the rollout forward a current bf16 fragment copy.  Hashed: the trajectory's action / log_prob / value."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from minppo_amd import _native as nat  # noqa: E402

LIB = Path(sys.argv[1]).resolve()
EMU = "emu" in LIB.name
f32 = np.float32
if EMU:
    lib, stream = nat.Lib(LIB), None

    def arr(x):
        x = np.ascontiguousarray(x)
        raw = np.zeros(x.nbytes + 256, np.uint8)
        o = (-raw.ctypes.data) % 256
        out = raw[o:o + x.nbytes].view(x.dtype).reshape(x.shape)
        out[...] = x
        return out

    ptr = lambda a: 0 if a is None else a.ctypes.data
    host = lambda a: np.array(a)
else:
    import torch

    nat.HIP_LIB_PATH = LIB
    lib = nat.load()
    _stream = torch.cuda.Stream(device="cuda:0")
    stream = _stream.cuda_stream
    arr = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to("cuda:0")
    ptr = lambda a: 0 if a is None else a.data_ptr()

    def host(a):
        _stream.synchronize()
        torch.cuda.synchronize()
        return a.detach().cpu().numpy()

full = lambda n, v, dt=f32: arr(np.full((n,), v, dt))


def show(case, **bufs):
    for k, v in bufs.items():
        print(f"{case} {k} {hashlib.sha256(np.ascontiguousarray(host(v)).tobytes()).hexdigest()}")


def lds_bytes(O, A, H):  # csrc/fused_common.h FusedLds, 16-row tiles
    KP, OT = (O + 31) // 32 * 32, 2 if A > 16 else 1
    return 4 * (16 * max(KP + 4, H + 4) + 2 * 16 * (H + 4) + 2 * 16 * 16 * OT + 16)


def setup(O, A, H, B, tanh, bf16, seed):
    rng = np.random.default_rng(seed)
    OP = (O + 3) // 4 * 4
    net = nat.Net(O, OP, A, H, tanh, bf16)
    P = lib.param_count(C.byref(net))
    flat = (rng.standard_normal(P) * 0.1).astype(f32)
    obs = np.zeros((B, OP), f32)
    obs[:, :O] = rng.standard_normal((B, O))
    d = dict(flat=flat, obs=obs, act=rng.standard_normal((B, A)).astype(f32), val=rng.standard_normal(B).astype(f32), lp=rng.standard_normal(B).astype(f32) - 5.0,
             adv=rng.standard_normal(B).astype(f32), tgt=rng.standard_normal(B).astype(f32), perm=rng.permutation(B).astype(np.int32),
             noise=rng.standard_normal((B, A)).astype(f32), stats=np.array([0.1, 0.9], f32))
    return net, OP, P, {k: arr(v) for k, v in d.items()}, d["perm"]


def training(O, A, H, mb, B, tanh, bf16, paths=("plain", "shadow", "pre"), rows=None):
    case = f"train O={O} A={A} H={H} mb={mb} {'bf16' if bf16 else 'f32'} {'tanh' if tanh else 'relu'}"
    net, OP, P, d, perm = setup(O, A, H, B, tanh, bf16, 7)
    idx = [arr(perm[:mb].copy()), arr(perm[mb:2 * mb].copy())]
    batch = nat.Batch(ptr(d["obs"]), OP, ptr(d["act"]), A, ptr(d["val"]), ptr(d["lp"]), ptr(d["adv"]), ptr(d["tgt"]))
    lc = nat.LossCfg(0.2, 0.5, 0.01)
    fused = C.c_int32(-1)
    lib.minibatch_path(C.byref(net), C.byref(batch), C.byref(fused))
    assert fused.value == 1, case + ": not on the fused path"
    if rows is not None:
        r = C.c_int32(0)
        lib.minibatch_rows_per_workgroup(C.byref(net), mb, 1, C.byref(r))
        assert r.value == rows, f"{case}: {r.value} rows per workgroup, expected {rows}"
    wsb = lib.grad_ws_bytes(C.byref(net), mb)
    args = lambda i: (C.byref(net), ptr(d["flat"]), C.byref(batch), ptr(idx[i]))
    tail = lambda g, l, ws: (mb, ptr(d["stats"]), 1.0 / mb, C.byref(lc), ptr(g), ptr(l), ptr(ws), wsb)
    if "plain" in paths:
        ws, g, l = full(wsb // 4 + 4, np.nan), full(P, np.nan), full(4, 0.0)
        lib.minibatch_grad(*args(0), *tail(g, l, ws), stream)
        show(case + " grad", ws=ws, grad=g, loss4=l)
    if "shadow" in paths:
        ws, g, l = full(wsb // 4 + 4, np.nan), full(P, np.nan), full(4, 0.0)
        lib.shadow_refresh(C.byref(net), ptr(d["flat"]), mb, ptr(ws), wsb, stream)
        lib.minibatch_grad_shadow(*args(0), *tail(g, l, ws), stream)
        show(case + " grad_shadow", ws=ws, grad=g, loss4=l)
    if "pre" in paths:
        ws = full(wsb // 4 + 4, np.nan)
        lib.shadow_refresh(C.byref(net), ptr(d["flat"]), mb, ptr(ws), wsb, stream)
        lib.gather_rows(C.byref(net), C.byref(batch), ptr(idx[0]), mb, ptr(ws), wsb, 0, stream)
        for parity in (0, 1):
            g, l = full(P, np.nan), full(4, 0.0)
            lib.minibatch_grad_pre(*args(parity), ptr(idx[1]) if parity == 0 else 0, *tail(g, l, ws), parity, stream)
            show(case + f" grad_pre parity={parity}", ws=ws, grad=g, loss4=l)


def rollout(O, A, H, n, tanh, bf16):
    case = f"rollout O={O} A={A} H={H} n={n} {'bf16' if bf16 else 'f32'} {'tanh' if tanh else 'relu'}"
    net, OP, P, d, _ = setup(O, A, H, n, tanh, bf16, 9)
    AP = (A + 3) // 4 * 4
    wsb = lib.policy_ws_bytes(C.byref(net), n)
    for mode in ("noise+value", "value"):
        act, logp, value, mean, ws = full(n * A, np.nan), full(n, np.nan), full(n, np.nan), full(n * AP, np.nan), full(wsb // 4 + 4, np.nan)
        sample = mode != "value"
        lib.policy_forward(C.byref(net), ptr(d["flat"]), n, ptr(d["obs"]), OP, ptr(d["noise"]) if sample else 0, ptr(act) if sample else 0,
                           ptr(logp) if sample else 0, ptr(value), ptr(mean) if sample else 0, ptr(ws), wsb, stream)
        show(f"{case} {mode}", action=act, log_prob=logp, value=value, mean_out=mean)


def engine(dtype):
    from minppo_amd.config import load_config_from_cli
    from minppo_amd.train import Trainer

    cfg = load_config_from_cli(["stompy_pro", "training.num_envs=64", "training.num_minibatches=4", "training.update_epochs=2", "training.mlp_dtype=" + dtype])
    tr = Trainer(cfg, lib=lib, xp="numpy", use_graph=False) if EMU else Trainer(cfg, use_graph=False)
    tr.reset()
    for k in (0, 1):
        tr.rollout()
        tr._sync()
        tj = tr.traj()
        show(f"engine stompy_pro {dtype} rollout {k}", **{n: (tj[n] if EMU else tj[n].detach()) for n in ("action", "log_prob", "value")})
        if k == 0:
            tr.learn()
    tr.close()


for O, A, H, mb in ((37, 5, 64, 42), (37, 5, 64, 48), (37, 20, 64, 48)):
    for bf16 in (0, 1):
        for tanh in (1, 0):
            training(O, A, H, mb, 96, tanh, bf16)
for A in (5, 20):
    if EMU:
        training(37, A, 64, 64, 128, 1, 0, paths=("pre",), rows=32)
    else:
        training(37, A, 256, 2080, 4160, 1, 0, paths=("pre",), rows=32)
for O, A, H in ((37, 5, 64), (37, 20, 64)):
    for bf16 in (0, 1):
        for tanh in (1, 0):
            rollout(O, A, H, 33, tanh, bf16)
for O in (415, 447):
    print(f"# O={O} A=20 H=256: {lds_bytes(O, 20, 256)} bytes of LDS per workgroup")
    for bf16 in (0, 1):
        training(O, 20, 256, 48, 96, 1, bf16)
        rollout(O, 20, 256, 33, 1, bf16)
if "--no-engine" not in sys.argv:
    for dtype in ("bf16", "f32"):
        engine(dtype)
