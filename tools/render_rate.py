"""What a rendered frame costs on one MI355X.

    python tools/render_rate.py [--out profiles/render_rate.txt]

`mppo_render` of 256 frames of 640 x 480 in ONE call (two launches: poses, rays), rgb output only, for synth_stompy_pro and for the export-style
biped (tests/golden/export_biped/robot.xml: more visuals, mesh hulls), through the camera `track`.  The frames differ: the joints swing and the root drifts and turns
(no physics is needed to time a renderer).  After a warm-up, five repetitions of 20 back-to-back calls per robot, alternating between the two, timed with device
events around work that ends in a synchronise.  There is nothing to compare the time with - the parent of this tool cannot render - so the
figures stand alone: time per frame, rays per second (primary rays; a lit hit casts a shadow ray through the same loop), and what bounds it.

    python tools/render_rate.py --grid 16 --samples 4 [--out profiles/render_grid_rate.txt]

`mppo_render_grid` (synth_stompy_pro, camera `track`), two comparisons in one process, alternating, timed the same way:
  the grid   256 frames of a grid of E = 16 environments (4 x 4 cells of 160 x 120, one sample) in one call, against the same 4096 views as 4096
             separate 160 x 120 frames through `mppo_render` in one call - the same rays, the scene staged per 16 x 16 tile either way;
  samples    256 frames of ONE 640 x 480 view at S = 1 .. 4 (S x S rays per pixel), and `mppo_render` of the same frames: how far below S * S the
             S-fold cost stays (staging and the tile's prologue are paid once per S * S rays)."""
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
ap.add_argument("--out", default=None)
ap.add_argument("--grid", type=int, default=0, help="E > 0: time mppo_render_grid with E environments per frame instead")
ap.add_argument("--samples", type=int, default=1, help="with --grid: the largest S of the supersampling sweep (1 .. 4)")
args = ap.parse_args()
out = open(args.out or str(ROOT / "profiles" / ("render_grid_rate.txt" if args.grid else "render_rate.txt")), "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def swinging(cm, n):
    """n poses that differ: the joints swing, the root drifts and turns (no physics needed to time a renderer)"""
    rng = np.random.default_rng(0)
    q = np.tile(np.asarray(cm.t["qpos0"], np.float32), (n, 1))
    phase = np.linspace(0.0, 4.0 * np.pi, n, dtype=np.float32)
    for j in range(cm.njnt):
        qa, jt = int(cm.t["jnt_qposadr"][j]), int(cm.t["jnt_type"][j])
        if jt == 0:
            q[:, qa] += 0.3 * np.sin(phase)
            q[:, qa + 3] = np.cos(0.2 * np.sin(phase)); q[:, qa + 6] = np.sin(0.2 * np.sin(phase))
        elif jt != 1:
            q[:, qa] += 0.4 * np.sin(phase + rng.uniform(0, 6.28))
    return q


dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)


def timed(call, calls=CALLS):
    """ms for `calls` back-to-back calls: device events around work that ends in a synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(calls):
        call()
    b.record(stream)
    stream.synchronize()
    return a.elapsed_time(b) / calls


def grid_rate(E, smax):
    cm = load_model(ROBOTS[0])
    r = R.Renderer(cm, device=dev)
    cam, nq = R.camera_index(cm, "track"), cm.nq
    cols = int(np.ceil(np.sqrt(E)))
    rows = -(-E // cols)
    cw, ch = W // cols, H // rows
    qd = torch.from_numpy(swinging(cm, F * E)).to(dev)  # [F, E, nq] packed = F * E separate frames
    grid = torch.zeros((F, rows * ch, cols * cw, 3), dtype=torch.uint8, device=dev)
    sep = torch.zeros((F * E, ch, cw, 3), dtype=torch.uint8, device=dev)
    full = torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev)
    o_sep, o_full = nat.RenderOut(rgb=sep.data_ptr()), nat.RenderOut(rgb=full.data_ptr())
    lib, sc, st, q = r.lib, r._scene, stream.cuda_stream, qd.data_ptr()
    variants = [(f"grid {rows} x {cols} of {cw} x {ch} cells, S = 1 ({F} frames per call)", lambda: lib.render_grid(sc, F, E, q, E * nq, nq, cam, cols, cw, ch, 1, grid.data_ptr(), st)),
                (f"mppo_render, {F * E} separate {cw} x {ch} frames per call", lambda: lib.render(sc, F * E, q, nq, cam, cw, ch, C.byref(o_sep), st)),
                (f"mppo_render, {F} frames of {W} x {H} per call", lambda: lib.render(sc, F, q, E * nq, cam, W, H, C.byref(o_full), st))]
    for S in range(1, smax + 1):
        variants.append((f"one {W} x {H} view, S = {S} ({F} frames per call)", lambda S=S: lib.render_grid(sc, F, 1, q, E * nq, nq, cam, 1, W, H, S, full.data_ptr(), st)))
    torch.cuda.synchronize()
    for _, call in variants:  # warm-up: code objects, scratch allocation, clocks
        timed(call, 2)
    ms = [[] for _ in variants]
    for _ in range(5):  # alternating
        for k, (_, call) in enumerate(variants):
            ms[k].append(timed(call))
    say(f"# mppo_render_grid, {Path(ROBOTS[0]).name} ({r.dims.ngeom} visuals), camera track, rgb only; device events around {CALLS} back-to-back calls that end in a synchronise; "
        "5 alternating repetitions after a warm-up; ms per call")
    med = [float(np.median(m)) for m in ms]
    for (label, _), m, md in zip(variants, ms, med):
        say(f"{label}: " + " ".join(f"{x:.4f}" for x in m) + f"   median {md:.4f}")
    say(f"# grid S = 1 / separate frames: {med[0] / med[1]:.3f}")
    base = med[3]
    say(f"# one view, S = 1 / mppo_render: {base / med[2]:.3f}")
    for S in range(2, smax + 1):
        say(f"# S = {S}: {med[2 + S] / base:.2f} x the S = 1 time for {S * S} x the rays ({W * H * S * S * F / med[2 + S] / 1e6:.1f} G primary rays/s)")
    # the two paths must draw the same picture: S = 1 grid cells against the separate frames, bit for bit
    lib.render_grid(sc, F, E, q, E * nq, nq, cam, cols, cw, ch, 1, grid.data_ptr(), st)
    lib.render(sc, F * E, q, nq, cam, cw, ch, C.byref(o_sep), st)
    stream.synchronize()
    cells = grid.cpu().numpy().reshape(F, rows, ch, cols, cw, 3).transpose(0, 1, 3, 2, 4, 5).reshape(F, rows * cols, ch, cw, 3)[:, :E]
    say(f"# grid cells equal the separate frames bit for bit: {bool(np.array_equal(cells.reshape(F * E, ch, cw, 3), sep.cpu().numpy()))}")
    r.close()


if args.grid:
    if not 1 <= args.samples <= 4:
        raise SystemExit("--samples: 1 .. 4")
    grid_rate(args.grid, args.samples)
    out.close()
    sys.exit(0)

runs = []
for name in ROBOTS:
    cm = load_model(name)
    r = R.Renderer(cm, device=dev)
    q = swinging(cm, F)
    qd = torch.from_numpy(q).to(dev)
    rgb = torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev)
    o = nat.RenderOut(rgb=rgb.data_ptr())
    cam = R.camera_index(cm, "track")
    torch.cuda.synchronize()

    def run(r=r, qd=qd, o=o, cam=cam, nq=cm.nq):
        return timed(lambda: r.lib.render(r._scene, F, qd.data_ptr(), nq, cam, W, H, C.byref(o), stream.cuda_stream)) / F  # ms per frame

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
