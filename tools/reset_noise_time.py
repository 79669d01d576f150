"""What `environment.reset_noise_scale` costs: the update with and without it, and the masked reset launch on its own (HIP events), at the headline shape
(stompy_pro, 4096 environments) and at the export biped (tests/golden/export_biped, 33 dofs).

    python tools/reset_noise_time.py [updates]                                        # HIP events
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/reset_noise_time.py 10  # the kernels' own times (a run of its own)

The reference's healthy band never ends an episode at these shapes (profiles/r03_f_training_run_1B.log), so the update at scale 0.01 shows what the T
masked launches cost when no workgroup has anything to do; the stand-alone launches are timed with no, one, 1 % and all environments masked in.
profiles/reset_noise_env_time.txt holds its output, the trace's env_kernel figures and a bench.py A/B of the same session."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from minppo_amd import _native as nat  # noqa: E402
from minppo_amd.config import load_config_from_cli  # noqa: E402
from minppo_amd.train import Trainer  # noqa: E402

UPDATES = int(sys.argv[1]) if len(sys.argv) > 1 else 30
BIPED = str(ROOT / "tests" / "golden" / "export_biped" / "robot.xml")
CASES = [("stompy_pro (headline shape)", ["stompy_pro", "training.num_envs=4096"]),
         ("export biped", ["stompy_pro", f"environment.model={BIPED}", "training.num_envs=4096"])]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3  # microseconds


for name, args in CASES:
    per_update = {}
    for scale in (0.0, 0.01, 0.0, 0.01):  # alternating: two readings each
        tr = Trainer(load_config_from_cli(args + [f"environment.reset_noise_scale={scale}"]), device="cuda:0")
        tr.reset()
        for _ in range(3):
            tr.update()
        tr._sync()
        torch.cuda.synchronize()
        with torch.cuda.stream(tr.stream):
            us = timed(tr.update, UPDATES)
        done = float(tr.region("done").float().mean())
        per_update.setdefault(scale, []).append(us)
        N, T = tr.N, tr.T
        print(f"{name}: N={N} T={T} reset_noise_scale={scale}: {us:9.1f} us per update ({N * T / us:6.3f} M env-steps/s), graph {'replayed' if tr.graph_active() else 'not used'}, "
              f"{100 * done:.3f} % of the last rollout's steps ended an episode", flush=True)
        if scale > 0 and len(per_update[scale]) == 2:
            # the masked launch on its own, on this trainer's model and state (after the timed updates)
            lib, h, dims = tr.lib, tr._model, tr.dims
            state, obs = tr.region("state"), tr.region("obs")
            s = tr._stream_ptr
            rng = np.random.default_rng(0)
            for label, mask in (("no environment masked in", np.zeros(N, np.uint8)), ("one environment", np.eye(1, N, N // 2, dtype=np.uint8)[0]),
                                ("1 % of the environments", (rng.random(N) < 0.01).astype(np.uint8)), ("every environment", np.ones(N, np.uint8))):
                dmask = torch.from_numpy(mask).to(tr.device)
                launch = lambda: lib.env_reinit(h, N, state.data_ptr(), obs.data_ptr(), dims.obs_pad, dmask.data_ptr(), scale, 0, 1337, 0, 0, 0, 5, s)
                with torch.cuda.stream(tr.stream):
                    timed(launch, 5)
                    us = timed(launch, 50)
                print(f"{name}: masked reset launch, {label} ({int(mask.sum())} of {N}): {us:7.2f} us per launch (back to back, HIP events)", flush=True)
        tr.close()
    a, b = (sum(per_update[k]) / len(per_update[k]) for k in (0.0, 0.01))
    print(f"{name}: update at scale 0.01 - update at scale 0 = {b - a:+.1f} us ({100 * (b - a) / a:+.2f} %), T = {T} masked launches: {(b - a) / T:+.2f} us each", flush=True)
