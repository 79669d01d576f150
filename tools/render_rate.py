"""What a rendered frame costs on one MI355X.

    python tools/render_rate.py [--out profiles/render_rate.txt]

`mppo_render` of 256 frames of 640 x 480 in ONE call (two launches: poses, rays), rgb output only, for synth_stompy_pro and for the export-style
biped (tests/golden/export_biped/robot.xml: more visuals, mesh hulls), through the camera `track`.  The frames differ: the joints swing and the root drifts and turns
(no physics is needed to time a renderer).  After a warm-up, five repetitions of 20 back-to-back calls per robot, alternating between the two, timed with device
events around work that ends in a synchronise.  There is nothing to compare the time with - the parent of this tool cannot render - so the
figures stand alone: time per frame, rays per second (primary rays; a lit hit casts a shadow ray through the same loop), and what bounds it."""
import argparse
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from minppo_amd import _native as nat
from minppo_amd import render as R
from minppo_amd.model import load_model

F, W, H = 256, 640, 480
CALLS = 20  # per timed window: back to back, so that a window is tens of milliseconds of device work
ROBOTS = ["synth_stompy_pro", str(ROOT / "tests" / "golden" / "export_biped" / "robot.xml")]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "render_rate.txt"))
out = open(ap.parse_args().out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
runs = []
for name in ROBOTS:
    cm = load_model(name)
    r = R.Renderer(cm, device=dev)
    rng = np.random.default_rng(0)
    # frames that differ: the joints swing, the root drifts and turns (no physics needed to time a renderer)
    q = np.tile(np.asarray(cm.t["qpos0"], np.float32), (F, 1))
    phase = np.linspace(0.0, 4.0 * np.pi, F, dtype=np.float32)
    for j in range(cm.njnt):
        qa, jt = int(cm.t["jnt_qposadr"][j]), int(cm.t["jnt_type"][j])
        if jt == 0:
            q[:, qa] += 0.3 * np.sin(phase)
            q[:, qa + 3] = np.cos(0.2 * np.sin(phase)); q[:, qa + 6] = np.sin(0.2 * np.sin(phase))
        elif jt != 1:
            q[:, qa] += 0.4 * np.sin(phase + rng.uniform(0, 6.28))
    qd = torch.from_numpy(q).to(dev)
    rgb = torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev)
    o = nat.RenderOut(rgb=rgb.data_ptr())
    cam = R.camera_index(cm, "track")
    torch.cuda.synchronize()

    def run(r=r, qd=qd, o=o, cam=cam, nq=cm.nq):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(CALLS):
            r.lib.render(r._scene, F, qd.data_ptr(), nq, cam, W, H, C.byref(o), stream.cuda_stream)
        b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) / (F * CALLS)  # ms per frame

    run()  # warm-up: code object, scratch allocation, clocks
    runs.append((name, cm, r, run, rgb, []))
for _ in range(5):  # alternating
    for name, cm, r, run, rgb, ms in runs:
        ms.append(run())
say(f"# mppo_render: {F} frames of {W} x {H} in one call (rgb only), camera track; device events around work that ends in a synchronise; 5 alternating repetitions of {CALLS} calls after a warm-up")
for name, cm, r, run, rgb, ms in runs:
    med = float(np.median(ms))
    img = rgb.cpu().numpy()
    colours = len(np.unique(img[F // 2].reshape(-1, 3), axis=0))
    say(f"{Path(name).name}: {r.dims.ngeom} visuals, {r.dims.nbody} bodies   ms/frame: " + " ".join(f"{x:.4f}" for x in ms) +
        f"   median {med:.4f}   -> {1e3 / med:.0f} frames/s, {W * H / med / 1e6:.2f} G primary rays/s   (frame {F // 2}: {colours} distinct colours, "
        f"{(img[F // 2] != img[0]).any(-1).mean() * 100:.1f} % of pixels differ from frame 0)")
    r.close()
say("# what bounds it (from the two figures, not from counters): the per-visual intersection loop - every lane visits every visual, twice where a lit hit casts its "
    f"shadow ray, and the time grows with the number of visuals; the image write is {W * H * 3 / 1e6:.2f} MB per frame, which HBM takes in well under a microsecond")
out.close()
