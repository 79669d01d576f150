"""The tiled many-environment view with supersampling (`mppo_render_grid`, `render_grid_rays_kernel<S>`, `Renderer.render_grid`, `samples=`), on the
emulator build and (marked gpu) on the HIP library.  Cells of 21 x 13 pixels (two 16 x 16 tiles across, one partial, and a partial tile down), E = 3 in 2
columns (one blank cell), F = 2; a scene with every shape and the ground under a fixed camera, a built-in robot under `track`.  S = 1 is held to
`mppo_render`'s image of every environment, bit for bit.  S = 2, 3 are held to tests/render_oracle.py at (S * 21, S * 13), its uint8 rgb box-averaged over
S x S blocks in float64, on the pixels all of whose sub-samples are in `render_oracle.compared`'s mask: each unstable sub-sample excludes at most one pixel,
so at most S * S * 1 % of an image may be excluded (asserted of the oracle alone).  Bound: 1.5 levels - averaging the oracle's rounded sub-samples moves the
mean by at most 0.5, the kernel's own rounding adds at most 0.5, float32 shading error on mask-stable rays is orders below a level."""
import functools

import numpy as np
import pytest

import render_oracle as ro
from minppo_amd import _native as nat
from minppo_amd import mjcf
from minppo_amd import model as M
from minppo_amd import render as R
from minppo_amd.config import make_config

BASE = {"kscale_id": "5eb3cb7f23232298", "visualization": {"camera_name": "track"}}
CW, CH, F, E, COLS, N, MAX_EXCLUDED, BOUND = 21, 13, 2, 3, 2, 5, 0.01, 1.5


def _every_shape():
    spec = M.synth_pile()  # box, hull, sphere, capsule, cylinder on the ground; plus an ellipsoid
    spec.world_visuals.append(M.VisualSpec(M.GEOM_ELLIPSOID, (0.25, 0.15, 0.1), pos=(0.5, 0.6, 0.35), rgba=(0.1, 0.8, 0.2, 1.0)))
    pos, target = np.array([0.6, -2.2, 2.6]), np.array([0.45, 0.4, 0.1])
    z = M._normalize(pos - target)
    x = M._normalize(np.cross([0.0, 0.0, 1.0], z))
    spec.cameras.append(M.CameraSpec("above", "world", "fixed", tuple(pos), tuple(mjcf._mat_to_quat(np.stack([x, np.cross(z, x), z], axis=1))), 45.0))
    return M.compile_model(spec)


def _robot():
    spec = M.BUILTIN_MODELS["synth_stompy_pro"]()
    spec.world_visuals.append(M.VisualSpec(M.GEOM_BOX, (6.0, 0.1, 1.5), pos=(0.0, 2.5, 1.5), rgba=(0.6, 0.5, 0.4, 1.0)))  # a wall: no far checker under a horizon
    return M.compile_model(spec)


SCENES = {"shapes": (_every_shape, "above", 0.03, 0.12, 0.25), "robot": (_robot, "track", 0.25, 0.3, 0.6)}


@functools.lru_cache(maxsize=None)
def scene(name):  # -> (compiled model, camera name, qpos [F, E, nq] float32: qpos0 moved differently per frame and environment)
    make, cam, dpos, dquat, dq = SCENES[name]
    cm, rng = make(), np.random.default_rng(11)
    q = np.tile(np.asarray(cm.t["qpos0"], np.float64), (F, E, 1))
    for j in range(cm.njnt):
        qa = int(cm.t["jnt_qposadr"][j])
        if int(cm.t["jnt_type"][j]) == M.JNT_FREE:
            q[..., qa:qa + 3] += dpos * rng.normal(size=(F, E, 3))
            q[..., qa + 3:qa + 7] += dquat * rng.normal(size=(F, E, 4))  # (not normalised: the kernel normalises)
        else:
            q[..., qa] += dq * rng.normal(size=(F, E))
    return cm, cam, q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, S):  # -> (box-averaged float64 oracle image [F, E, CH, CW, 3], compared pixels [F, E, CH, CW]); asserts the cap on excluded pixels
    cm, cam, q = scene(name)
    per = [ro.compared(cm, q[:, e], R.camera_index(cm, cam), S * CW, S * CH) for e in range(E)]
    mean = np.stack([ref["rgb"].reshape(F, CH, S, CW, S, 3).astype(np.float64).mean((2, 4)) for ref, _ in per], 1)
    mask = np.stack([m.reshape(F, CH, S, CW, S).all((2, 4)) for _, m in per], 1)
    share = 1.0 - mask.reshape(F, E, -1).mean(-1)
    print(f"{name} S={S}: excluded share per image {share.ravel()}")
    assert (share <= S * S * MAX_EXCLUDED).all(), (name, S, share)
    return mean, mask


def draw(be, name, samples, layout="packed", cols=COLS, envs=E):
    cm, cam, q = scene(name)
    rec_dim = ((cm.nq + 2 * cm.nv + 16 * (cm.nbody - 1) + 3) & ~3) + ((cm.nv + 2 + 3) & ~3)  # (include/minppo_hip.h, "Persistent per-env record")
    if layout == "records":  # the first E of N state records per frame, drawn in place: q_ld_env = rec_dim, q_ld_frame = N * rec_dim
        rows = np.full((F, N, rec_dim), 7.25, np.float32)
        rows[:, :E, :cm.nq] = q
        q = be.arr(rows)[:, :E]
    with R.Renderer(cm, lib=be.lib, xp=be.xp, **({} if be.name == "emu" else {"device": "cuda:0"})) as r:
        single = [r.render(q[:, e], cam, CW, CH) for e in range(E)] if samples == 1 else None
        return r.render_grid(q[:, :envs], cam, CW, CH, cols=cols, samples=samples), single, r.render(q[:, 0], cam, CW, CH, samples=samples)


def cells(img):  # [F, rows * CH, COLS * CW, 3] -> [F, rows * COLS, CH, CW, 3]
    return img.reshape(F, -1, CH, COLS, CW, 3).transpose(0, 1, 3, 2, 4, 5).reshape(F, -1, CH, CW, 3)


@pytest.mark.parametrize("layout", ["packed", "records"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_one_sample_is_the_single_view_renderer_bit_for_bit(be, name, layout):
    got, single, _ = draw(be, name, 1, layout)
    assert got.shape == (F, 2 * CH, COLS * CW, 3) and got.dtype == np.uint8
    c = cells(got)
    assert [np.array_equal(c[:, e], single[e]) for e in range(E)] == [True] * E
    assert len({single[e].tobytes() for e in range(E)}) == E  # (the environments differ)
    assert np.array_equal(c[:, E], np.broadcast_to(np.floor(255.0 * np.asarray(ro.SKY) + 0.5).astype(np.uint8), (F, CH, CW, 3)))


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_supersampled_cells_equal_the_box_filtered_float64_ray_caster(be, name, S):
    mean, mask = reference(name, S)
    got = cells(draw(be, name, S)[0])[:, :E].astype(np.float64)
    err = np.abs(got - mean)[mask]
    print(f"{be.name} {name} S={S}: largest difference {err.max():.3f} levels on {mask.mean() * 100:.1f} % of the pixels (allowed {BOUND})")
    assert err.max() <= BOUND, err.max()


@pytest.mark.parametrize("bad,msg", [(dict(samples=5), "samples = 5"), (dict(cols=0), "cols = 0"), (dict(E=0), "E = 0")])
def test_bad_arguments_are_refused_with_a_message(be, bad, msg):
    cm, cam, q = scene("shapes")
    a = {"E": E, "cols": COLS, "samples": 1, **bad}
    qd, rgb = be.arr(q), be.zeros((F, 2 * CH, COLS * CW, 3), np.uint8)
    with R.Renderer(cm, lib=be.lib, xp=be.xp, **({} if be.name == "emu" else {"device": "cuda:0"})) as r:
        with pytest.raises(nat.NativeError, match=msg):
            be.lib.render_grid(r._scene, F, a["E"], be.ptr(qd), E * cm.nq, cm.nq, R.camera_index(cm, cam), a["cols"], CW, CH, a["samples"], be.ptr(rgb), be.stream)


def test_evaluation_video_grid_draws_every_recorded_environment(be, tmp_path):
    from minppo_amd.evaluate import evaluate
    from minppo_amd.train import init_flat_params

    kw = {} if be.name == "emu" else {"device": "cuda:0"}
    cfg = make_config(BASE, ["model.hidden_size=64", "evaluation.num_envs=4", "evaluation.num_steps=2", "evaluation.record_envs=3", "evaluation.video_grid=true",
                             f"evaluation.video_path={tmp_path / 'grid.npz'}", f"visualization.width={CW}", f"visualization.height={CH}", "visualization.samples=2"])
    res = evaluate(cfg, init_flat_params(3, 225, 10, 64), lib=be.lib, xp=be.xp, **kw)
    frames = np.load(tmp_path / "grid.npz")["frames"]
    assert frames.shape == (2, 2 * CH, 2 * CW, 3)
    want = [R.render(M.load_model("synth_stompy_pro"), res.trajectory["qpos"][:2, e], "track", CW, CH, samples=2, lib=be.lib, xp=be.xp, **kw) for e in range(3)]
    assert [np.array_equal(cells(frames)[:, e], want[e]) for e in range(3)] == [True] * 3


@pytest.mark.gpu
def test_humanoid_env_renders_chosen_environments_as_a_grid():
    import torch

    from minppo_amd.env import HumanoidEnv

    env = HumanoidEnv(make_config(BASE))
    try:
        first = es = env.reset(num_envs=4)
        for _ in range(20):  # (every environment under an action of its own: different poses)
            es = env.step(es, torch.linspace(-1, 1, 4, device=env.device)[:, None].expand(4, env.action_size).contiguous())
        states = [first, es]
        got = cells(env.render(states, width=CW, height=CH, envs=[2, 0, 3], cols=COLS))
        single = [env.render(states, width=CW, height=CH, env_index=e) for e in (2, 0, 3)]
        assert [np.array_equal(got[:, k], single[k]) for k in range(3)] == [True] * 3 and not np.array_equal(single[0], single[1])
    finally:
        env.close()


def test_surface_default_columns_and_single_view_samples(be):
    auto, _, one = draw(be, "robot", 2, cols=None)  # E = 3: ceil(sqrt(3)) = 2 columns
    assert auto.shape == (F, 2 * CH, 2 * CW, 3) and np.array_equal(auto, draw(be, "robot", 2)[0])
    single = draw(be, "robot", 2, cols=None, envs=1)[0]  # E = 1: one cell
    assert single.shape == (F, CH, CW, 3) and np.array_equal(one, single) and np.array_equal(one, cells(auto)[:, 0])
