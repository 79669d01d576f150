"""`minppo evaluate` - run a trained policy: deterministic (or sampled) rollouts, episode statistics, joint trajectories.

The reference stops at a stub (`minppo/infer.py:22-27` raises NotImplementedError) and its environment has no time limit
(`env.py:238-242` ends an episode on height only), so a policy that stands never finishes an episode.  `evaluate` therefore runs a
fixed horizon - `evaluation.num_steps` steps of `evaluation.num_envs` environments - as ONE call into the engine (`mppo_evaluate`,
csrc/evaluator.hip: policy forward, environment step, statistics and trajectory rows all on the device) and reports both the
episodes that ended and the environments that never fell.

    python -m minppo_amd.cli evaluate <config> inference.model_path=trained_model.pkl [evaluation.num_envs=256 ...]

prints one JSON line with the statistics; `evaluation.trajectory_path=run.npz evaluation.record_envs=4` also writes the joint
trajectory of the first four environments (`qpos`, `qvel`, `action`, `reward`, `done`, and `dt`, `n_frames`); `evaluation.video_path=policy.avi`
(with `record_envs >= 1`) renders recorded environment 0 - one frame per step, camera and size from `visualization` - and writes the video
(minppo_amd/render.py: train, then watch it).

Under random pushes (`environment.push_force` > 0 with `push_interval`, `push_duration`, `push_body`) the same call goes through
`mppo_evaluate_push`: every environment is shoved on `push_duration` of every `push_interval` steps, and `survivors` of `num_envs` - the
environments that never fell - is the robustness figure two standing policies are compared by.  The wrench of any (environment, step) is
`minppo_amd.jaxrng.push_wrench_philox(seed, 0, step, num_envs, push_force, push_interval, push_duration)[environment]`.  The result, its JSON line
and the trajectory file are what they are without pushes.

Under an episode time limit (`environment.episode_length` = L > 0) the call goes through `mppo_evaluate_limit`: an environment whose episode
reaches L steps is truncated and restarts, as in training (without the stagger).  The episode statistics then include the truncated episodes, and the
result - and its JSON line - gain `truncated_episodes` (the episodes the limit cut) and `falls` (the episodes that ended in a fall: `episodes` minus those);
`survivors` is the number of environments that never FELL (without a limit that is the same thing as "none of its episodes ended") and
`survivor_mean_return` is null (a survivor's return is spread over its truncated episodes, which `mean_return` already covers).  The trajectory's
`done` column includes the truncations.

Under sensor noise (`environment.obs_noise_level` > 0) and actuation latency (`environment.action_delay_max` > 0) the call goes through
`mppo_evaluate_sensors` - "does it still stand with 20 ms of latency and noisy encoders?" - under `deterministic` too; the JSON line echoes the keys that are
on, and under a latency the trajectory gains `applied_action` (what the actuators were given; `action` stays the policy's own).
"""

from __future__ import annotations

import ctypes as C
import json
import logging
import math
import os
import sys
from dataclasses import asdict, dataclass
from typing import Any, Dict, Optional, Sequence

import numpy as np

from minppo_amd import _native as nat
from minppo_amd.config import Config, load_config_from_cli, require

logger = logging.getLogger(__name__)

_NAN = float("nan")


@dataclass
class EvalResult:
    """Statistics of one evaluation, derived on the host from the engine's `mppo_eval_result_t`.  The episode fields describe the
    episodes that ENDED within the horizon and are nan when none did; `survivors` counts the environments none of whose episodes
    ended, `survivor_mean_return` is the mean of the returns they collected over the whole horizon."""

    episodes: int
    mean_return: float
    std_return: float
    min_return: float
    max_return: float
    mean_length: float
    min_length: float
    max_length: float
    survivors: int
    survivor_mean_return: float
    mean_reward: float
    steps: int
    domain: Optional[Dict[str, float]] = None  # under domain randomisation only: the six numbers of its ranges (None without it: the key set is what it was)
    sensors: Optional[Dict[str, float]] = None  # under sensor noise / actuation latency only: the keys that are on (None without either)
    truncated_episodes: Optional[int] = None  # under an episode time limit only (None without one: the statistics' key set is then what it always was)
    falls: Optional[int] = None
    trajectory: Optional[Dict[str, np.ndarray]] = None
    dt: float = _NAN      # seconds per environment step (the model's timestep x n_frames): what a viewer needs beside the trajectory
    n_frames: int = 1

    def stats(self) -> Dict[str, Any]:
        """The statistics alone (what the command line prints)."""
        d = asdict(self)
        for k in ("trajectory", "dt", "n_frames"):
            d.pop(k)
        for k in ("truncated_episodes", "falls"):
            if d[k] is None:
                d.pop(k)
        dom = d.pop("domain")
        if dom is not None:  # (the ranges the figures belong to: a robustness sweep's lines say what they measured)
            d.update(dom)
        sens = d.pop("sensors")
        if sens is not None:  # (likewise: the noise and the latency the figures were measured under)
            d.update(sens)
        return d


def result_from_struct(r: nat.EvalResultRaw, trajectory: Optional[Dict[str, np.ndarray]] = None) -> EvalResult:
    n = int(r.episodes)
    if n > 0:
        mean = r.ret_sum / n
        std = math.sqrt(max(r.ret_sumsq / n - mean * mean, 0.0))  # population standard deviation of the ended episodes' returns
        ep = dict(mean_return=mean, std_return=std, min_return=float(r.ret_min), max_return=float(r.ret_max), mean_length=r.len_sum / n,
                  min_length=float(r.len_min), max_length=float(r.len_max))
    else:  # (the engine reports +inf / -inf and zeros there: nothing ended, nothing to average)
        ep = dict(mean_return=_NAN, std_return=_NAN, min_return=_NAN, max_return=_NAN, mean_length=_NAN, min_length=_NAN, max_length=_NAN)
    surv = int(r.survivors)
    return EvalResult(episodes=n, survivors=surv, survivor_mean_return=r.survivor_ret_sum / surv if surv > 0 else _NAN,
                      mean_reward=r.reward_sum / r.steps if r.steps > 0 else _NAN, steps=int(r.steps), trajectory=trajectory, **ep)


def split_trajectory(traj: np.ndarray, nq: int, nv: int, A: int) -> Dict[str, np.ndarray]:
    """[K + 1, R, nq + nv + A + 2] rows of `mppo_evaluate` -> named arrays (frame 0: the initial state, zero action / reward / done)."""
    return dict(qpos=traj[..., :nq].copy(), qvel=traj[..., nq:nq + nv].copy(), action=traj[..., nq + nv:nq + nv + A].copy(),
                reward=traj[..., nq + nv + A].copy(), done=traj[..., nq + nv + A + 1] != 0)


def _flat_params(params: Any, O: int, A: int, H: int, L: int) -> np.ndarray:
    from minppo_amd.train import param_slices, tree_to_flat

    if isinstance(params, (str, os.PathLike)):
        from minppo_amd.infer import load_model as load_pickle

        params = load_pickle(os.fspath(params))
    if isinstance(params, dict):
        return tree_to_flat(params, O, A, H, L)
    flat = np.ascontiguousarray(np.asarray(params), np.float32).reshape(-1)
    want = param_slices(O, A, H, L)[1]
    if flat.size != want:
        raise ValueError(f"expected {want} parameters (O = {O}, A = {A}, hidden_size = {H}, num_layers = {L}), got {flat.size}")
    return flat


def obs_norm_table(obs_norm: Optional[Dict[str, Any]], O: int):
    """The "obs_norm" entry of a model file (`Trainer.params` with `training.normalize_observations`) -> (float32 [2, O] table, clip); (None, 0.0) for None."""
    if obs_norm is None:
        return None, 0.0
    table = np.stack([np.asarray(obs_norm["mean"], np.float32).reshape(-1), np.asarray(obs_norm["inv_std"], np.float32).reshape(-1)])
    clip = float(obs_norm.get("clip", 0.0))
    if table.shape != (2, O):
        raise ValueError(f"obs_norm: mean / inv_std of {table.shape[1]} columns, the robot's observation has {O}")
    if not clip >= 0.0:
        raise ValueError(f"obs_norm: clip = {clip!r} cannot be negative")
    return np.ascontiguousarray(table), clip


def eval_cfg(config: Config, **overrides: Any) -> nat.EvalCfg:
    """`mppo_eval_cfg_t` of a config: sizes from `evaluation`, frames / reset noise from `environment`, the reward window from `reward`,
    the seed from `training.seed`.  Overrides: num_envs, num_steps, deterministic, record_envs, seed."""
    from minppo_amd.train import reward_cfg

    ev = config.evaluation
    unknown = set(overrides) - {"num_envs", "num_steps", "deterministic", "record_envs", "seed"}
    if unknown:
        raise TypeError(f"evaluate: unknown override(s) {sorted(unknown)}")
    g = lambda k, d: d if overrides.get(k) is None else overrides[k]
    return nat.EvalCfg(N=int(g("num_envs", ev.num_envs)), K=int(g("num_steps", ev.num_steps)), n_frames=int(config.environment.n_frames),
                       deterministic=int(bool(g("deterministic", ev.deterministic))), record_envs=int(g("record_envs", ev.record_envs)),
                       reset_noise_scale=float(config.environment.reset_noise_scale), seed=int(g("seed", config.training.seed)) & 0xFFFFFFFFFFFFFFFF,
                       reward=reward_cfg(config))


def run(lib: nat.Lib, xp: str, device: Any, stream: Any, model: C.c_void_p, dims: nat.ModelDims, net: nat.Net, params_dev: Any,
        ecfg: nat.EvalCfg, obs_norm: Optional[Dict[str, Any]] = None, push: Optional[nat.PushCfg] = None, episode_length: int = 0,
        domain: Optional[nat.DomainCfg] = None, obs_noise: Optional[np.ndarray] = None, action_delay: Optional[nat.ActionDelayCfg] = None) -> EvalResult:
    """One `mppo_evaluate` on an open model and parameters already in device memory (`Trainer.evaluate` comes in here); with `obs_norm`
    ({"mean", "inv_std", "clip"}) one `mppo_evaluate_obs_norm`: the policy reads observations normalised with that table; with `push`
    (`train.push_cfg`: random pushes, with or without a table) one `mppo_evaluate_push`; with `episode_length` > 0 (an episode time limit, with or
    without either) one `mppo_evaluate_limit`; with `domain` (`train.domain_cfg`: domain randomisation, with or without any of those) one
    `mppo_evaluate_domain`; with `obs_noise` (`train.obs_noise_scales`: float32 [O]) or `action_delay` (`train.action_delay_cfg`), with or without any of
    those, one `mppo_evaluate_sensors` - under a latency the trajectory then carries "applied_action"."""
    sensors = obs_noise is not None or action_delay is not None
    if obs_noise is not None:
        obs_noise = np.ascontiguousarray(obs_noise, np.float32).reshape(-1)
        if obs_noise.size != dims.obs_dim:
            raise ValueError(f"evaluate: obs_noise of {obs_noise.size} columns, the robot's observation has {dims.obs_dim}")
    table, clip = obs_norm_table(obs_norm, dims.obs_dim)
    limited = int(episode_length) > 0
    if int(episode_length) < 0:
        raise ValueError(f"evaluate: episode_length = {episode_length!r} cannot be negative")
    res_bytes = C.sizeof(nat.EvalResultRaw)  # (under a limit the second result lies behind the first in the same allocation)

    def call(ws, res, traj, s, traj_applied=None):
        if sensors:
            lib.evaluate_sensors(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), nat.ptr(ws), need, nat.ptr(table_dev), clip,
                                 C.byref(push) if push is not None else None, int(episode_length), C.byref(domain) if domain is not None else None,
                                 nat.ptr(obs_noise), C.byref(action_delay) if action_delay is not None else None, nat.ptr(res), nat.ptr(res) + res_bytes,
                                 nat.ptr(traj), nat.ptr(traj_applied), s)
        elif domain is not None:
            lib.evaluate_domain(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), nat.ptr(ws), need, nat.ptr(table_dev), clip,
                                C.byref(push) if push is not None else None, int(episode_length), C.byref(domain), nat.ptr(res), nat.ptr(res) + res_bytes,
                                nat.ptr(traj), s)
        elif limited:
            lib.evaluate_limit(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), nat.ptr(ws), need, nat.ptr(table_dev), clip,
                               C.byref(push) if push is not None else None, int(episode_length), nat.ptr(res), nat.ptr(res) + res_bytes, nat.ptr(traj), s)
        elif push is not None:
            lib.evaluate_push(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), nat.ptr(ws), need, nat.ptr(table_dev), clip, C.byref(push), nat.ptr(res),
                              nat.ptr(traj), s)
        elif table is None:
            lib.evaluate(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), nat.ptr(ws), need, nat.ptr(res), nat.ptr(traj), s)
        else:
            lib.evaluate_obs_norm(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), nat.ptr(ws), need, nat.ptr(table_dev), clip, nat.ptr(res), nat.ptr(traj), s)

    need = int((lib.eval_sensors_ws_bytes if sensors else lib.eval_domain_ws_bytes if domain is not None else lib.eval_limit_ws_bytes if limited else lib.eval_ws_bytes)(model, C.byref(net), C.byref(ecfg)))
    if need == 0:  # the arguments are ones mppo_evaluate refuses: let it say why
        lib.evaluate(model, C.byref(net), nat.ptr(params_dev), C.byref(ecfg), None, 0, None, None, None)
    K, R, nq, nv, A = ecfg.K, ecfg.record_envs, dims.nq, dims.nv, net.A
    W = nq + nv + A + 2
    if xp == "torch":
        import torch

        def alloc(nbytes):
            raw = torch.zeros(nbytes + 256, dtype=torch.uint8, device=device)
            o = (-raw.data_ptr()) % 256
            return raw[o:o + nbytes]

        ws, res = alloc(need), alloc(res_bytes + C.sizeof(nat.EvalLimitResultRaw))
        table_dev = torch.from_numpy(table).to(device) if table is not None else None
        traj = alloc((K + 1) * R * W * 4).view(torch.float32).reshape(K + 1, R, W) if R > 0 else None
        applied = alloc((K + 1) * R * A * 4).view(torch.float32).reshape(K + 1, R, A) if R > 0 and action_delay is not None else None
        with torch.cuda.device(device):
            torch.cuda.synchronize(device)  # (the allocations were zeroed on torch's current stream)
            call(ws, res, traj, stream.cuda_stream, applied)
            stream.synchronize()
        res_host = res.cpu().numpy()
        traj_host = traj.cpu().numpy() if traj is not None else None
        applied_host = applied.cpu().numpy() if applied is not None else None
    else:  # NumPy "device" memory: the CPU emulator build of the test-suite

        def alloc(nbytes):
            raw = np.zeros(nbytes + 256, np.uint8)
            o = (-raw.ctypes.data) % 256
            return raw[o:o + nbytes]

        ws, res_host = alloc(need), alloc(res_bytes + C.sizeof(nat.EvalLimitResultRaw))
        traj_host = alloc((K + 1) * R * W * 4).view(np.float32).reshape(K + 1, R, W) if R > 0 else None
        applied_host = alloc((K + 1) * R * A * 4).view(np.float32).reshape(K + 1, R, A) if R > 0 and action_delay is not None else None
        table_dev = table
        call(ws, res_host, traj_host, None, applied_host)
    out = result_from_struct(nat.EvalResultRaw.from_buffer_copy(res_host.tobytes()[:res_bytes]), split_trajectory(traj_host, nq, nv, A) if traj_host is not None else None)
    if applied_host is not None:  # (what the actuators were given; "action" stays the policy's own)
        out.trajectory["applied_action"] = np.array(applied_host)
    if limited:
        extra = nat.EvalLimitResultRaw.from_buffer_copy(res_host.tobytes()[res_bytes:])
        out.truncated_episodes = int(extra.truncated_episodes)
        out.falls = out.episodes - out.truncated_episodes
        out.survivors = int(ecfg.N) - int(extra.fallen_envs)  # the environments that never fell
        out.survivor_mean_return = _NAN
    out.dt, out.n_frames = float(dims.timestep) * ecfg.n_frames, int(ecfg.n_frames)
    return out


def evaluate(config: Config, params: Any, *, lib: Optional[nat.Lib] = None, xp: str = "torch", device: Any = "cuda:0", obs_norm: Optional[Dict[str, Any]] = None,
             **overrides: Any) -> EvalResult:
    """Evaluates `params` - the nested tree of `save_model` / `Trainer.params`, a flat vector, or the path of a `save_model` pickle - on
    the robot, network geometry, reward window and `evaluation` section of `config`.  `lib=` / `xp="numpy"` as in `Trainer`.
    A tree or pickle with an "obs_norm" entry (a policy trained with `training.normalize_observations`) is evaluated on observations normalised
    with it; `obs_norm=` ({"mean", "inv_std", "clip"}) supplies the entry for a flat vector or overrides the tree's.  A flat vector without it: none."""
    from minppo_amd.train import action_delay_cfg, domain_cfg, domain_echo, domain_on, obs_noise_scales, open_model, push_cfg, resolve_model, sensors_echo

    lib = lib if lib is not None else nat.load()
    if not 1 <= config.model.num_layers <= 4:
        raise ValueError(f"model.num_layers = {config.model.num_layers}: the MI355X engine lays out 1 to 4 hidden layers")
    ecfg = eval_cfg(config, **overrides)
    if config.evaluation.video_path and ecfg.record_envs < 1:  # (before anything runs)
        raise ValueError("evaluation.video_path is set but evaluation.record_envs is 0: there would be no trajectory to render")
    cm = resolve_model(config)
    torch, stream = None, None
    if xp == "torch":
        import torch

        device = torch.device(device)
        stream = torch.cuda.Stream(device=device)
    model, blob_host, blob_dev = open_model(lib, config, cm, xp, device)  # (the blobs live as long as the handle)
    try:
        dims = nat.ModelDims()
        lib.model_get_dims(model, C.byref(dims))
        L = int(config.model.num_layers)
        net = nat.Net(dims.obs_dim, dims.obs_pad, dims.nu, config.model.hidden_size, int(config.model.use_tanh), int(config.training.mlp_dtype == "bf16"), L)
        if isinstance(params, (str, os.PathLike)):
            from minppo_amd.infer import load_model as load_pickle

            params = load_pickle(os.fspath(params))
        if obs_norm is None and isinstance(params, dict):
            obs_norm = params.get("obs_norm")
        flat = _flat_params(params, dims.obs_dim, dims.nu, config.model.hidden_size, L)
        params_dev = torch.from_numpy(flat).to(device) if torch is not None else np.ascontiguousarray(flat)
        result = run(lib, xp, device, stream, model, dims, net, params_dev, ecfg, obs_norm=obs_norm, push=push_cfg(config, cm, ecfg.seed),
                     episode_length=int(config.environment.episode_length), domain=domain_cfg(config, cm, ecfg.seed),
                     obs_noise=obs_noise_scales(config, cm), action_delay=action_delay_cfg(config, ecfg.seed))
        result.sensors = sensors_echo(config) or None
        if domain_on(config):
            result.domain = domain_echo(config)
    finally:
        if torch is not None:
            torch.cuda.synchronize(device)
        lib.model_close(model)
    if config.evaluation.video_path:
        save_video(config.evaluation.video_path, config, result, lib=lib, xp=xp, device=device)
    return result


def save_trajectory(path: str, result: EvalResult) -> None:
    if result.trajectory is None:
        raise ValueError("save_trajectory: the evaluation recorded no environment (evaluation.record_envs = 0)")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:  # (an open file: np.savez appends ".npz" to a bare name)
        np.savez(f, dt=np.float64(result.dt), n_frames=np.int32(result.n_frames), **result.trajectory)


def save_video(path: str, config: Config, result: EvalResult, *, lib: Optional[nat.Lib] = None, xp: str = "torch", device: Any = "cuda:0") -> None:
    """Renders recorded environment 0's trajectory with `visualization.camera_name / width / height` and writes it to `path`
    (minppo_amd.render.write_video), at the frame rate of the environment step."""
    from minppo_amd.render import render, write_video
    from minppo_amd.train import resolve_model

    if result.trajectory is None:
        raise ValueError("save_video: the evaluation recorded no environment (evaluation.record_envs = 0)")
    vis = config.visualization
    # one frame per step: the state every step STARTED from (trajectory rows 0 .. K - 1; as env.py:302-303 collects a state before it steps)
    frames = render(resolve_model(config), result.trajectory["qpos"][:-1, 0], require(vis.camera_name, "visualization.camera_name"), vis.width, vis.height, lib=lib, xp=xp,
                    device=device)
    write_video(path, frames, fps=1.0 / result.dt)


def _json_value(v: Any) -> Any:
    return None if isinstance(v, float) and not math.isfinite(v) else v


def main(args: Sequence[str] | None = None) -> EvalResult:
    """`minppo evaluate <config> [overrides]`: evaluates the model file `inference.model_path` (the reference's own key) and prints one
    JSON line with the statistics (a statistic that does not exist - no episode ended - is null)."""
    if args is None:
        args = sys.argv[1:]
    config = load_config_from_cli(args)
    path = require(config.inference.model_path, "inference.model_path")
    if config.evaluation.trajectory_path and config.evaluation.record_envs < 1:  # (before anything runs)
        raise ValueError("evaluation.trajectory_path is set but evaluation.record_envs is 0: there would be no trajectory to write")
    if config.evaluation.video_path and config.evaluation.record_envs < 1:
        raise ValueError("evaluation.video_path is set but evaluation.record_envs is 0: there would be no trajectory to render")
    result = evaluate(config, path)
    if config.evaluation.trajectory_path:
        save_trajectory(config.evaluation.trajectory_path, result)
    print(json.dumps({k: _json_value(v) for k, v in result.stats().items()}), flush=True)
    return result


if __name__ == "__main__":
    main()
