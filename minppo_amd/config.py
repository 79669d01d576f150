"""Typed configuration tree for the MI355X-native minppo engine.

Mirrors the configuration *surface* of the reference (field names, defaults,
YAML + dot-list override grammar; reference `minppo/config.py:16-127`) without
OmegaConf, which is not available on the target image.  The merge order is the
reference's: structured defaults  <-  YAML file  <-  `a.b=c` dot-list overrides
(`minppo/config.py:120-123`).  The first positional argument is a path or a
bare config name resolved under `configs/` (`minppo/config.py:113-118`).

This module is host-side control plane: it is not accelerated and has no GPU
dependency.
"""

from __future__ import annotations

import dataclasses
import logging
import sys
from dataclasses import dataclass, field, fields, is_dataclass
from pathlib import Path
from typing import Any, Sequence

import yaml

logger = logging.getLogger(__name__)

CONFIG_ROOT_DIR = Path(__file__).parent / "configs"


class _Missing:
    """Sentinel for mandatory values (the reference uses `omegaconf.MISSING`)."""

    def __repr__(self) -> str:  # pragma: no cover - cosmetic
        return "???"

    def __bool__(self) -> bool:
        return False


MISSING: Any = _Missing()


class MissingMandatoryValue(ValueError):
    """Raised when a field that has no default is read before being set."""


@dataclass
class EnvironmentConfig:
    n_frames: int = field(default=1)
    backend: str = field(default="mjx")
    include_c_vals: bool = field(default=True)
    # Extension (not in the reference): name of a built-in robot model or path to
    # an MJCF file.  The reference downloads the MJCF by `kscale_id`; there is no
    # network on the target, so the engine resolves `kscale_id` through a local
    # table (minppo_amd/model.py) unless this is set.
    model: str = field(default="")
    # Extension: compile the environment kernel for THIS robot's dimensions at start-up (minppo_amd/jit.py: hipcc, about 20 s once,
    # cached) - the counterpart of the reference's jax.jit of its step function (env.py:123,147; train.py:306).  Bit-identical results (checked on the device
    # before use), 1.2x - 1.6x faster than the run-time-sized kernel; no effect for the robots the library was built for.
    jit_kernel: bool = field(default=False)
    # Extension: `HumanoidEnv.reset_noise_scale` (env.py:87, a class attribute the reference ships at 0) as a config key.  Above 0 every environment
    # starts, and restarts after `done`, from qpos0 + U(-s, s) / qvel = U(-s, s) (env.py:115-121; 1e-2 is customary for Brax humanoids), drawn inside
    # the environment kernel from the stream `training.rng_impl` names (threefry: the reference's own keys, train.py:135,142,163-165).  0: every
    # environment restarts from the one constant state, as before.  Negative: ValueError.
    reset_noise_scale: float = field(default=0.0)
    # Extension (absent upstream; legged_gym `push_robots`, MuJoCo Playground's push perturbation): random pushes.  Above 0, every environment is shoved
    # for `push_duration` of every `push_interval` env steps - out of phase with the others - by a horizontal force on `push_body` (a body name of the
    # model; "": body 1, the first root), each component uniform in [-push_force, push_force] newtons and constant for the shove (at the
    # built-in robots' 2 ms step the defaults are a 0.1 s shove every 2 s).  In training, in `evaluate` - whose `survivors` is then a robustness figure -
    # and in the `env` rollout.  The other three keys are read only when push_force > 0.  0: nothing changes.
    push_force: float = field(default=0.0)
    push_interval: int = field(default=1000)
    push_duration: int = field(default=50)
    push_body: str = field(default="")
    # Extension (absent upstream: env.py:238-242 ends an episode on height only; Brax `EpisodeWrapper(episode_length=1000)`, legged_gym, MuJoCo Playground):
    # an episode time limit in env steps.  An environment whose episode reaches it is TRUNCATED - restarted as a fallen one is, counted as an episode with its
    # return and length, and cut out of GAE (advantage 0, target = value: reaching the limit is no failure) - so a standing policy keeps producing episode
    # statistics and keeps seeing randomised starts.  In training, in `evaluate` and in `HumanoidEnv.step` / the `env` rollout.
    # `episode_length_stagger` (read only when episode_length > 0; training only): every environment's FIRST episode is cut at a length of its own, drawn in
    # 1 .. episode_length, so that the batch does not reach the limit in the same step for ever.  0: no limit, nothing changes.  Negative: ValueError.
    episode_length: int = field(default=0)
    episode_length_stagger: bool = field(default=True)
    # Extension (absent upstream; legged_gym `randomize_friction` / `randomize_base_mass` / motor strength, MuJoCo Playground and Brax `domain_randomize`):
    # domain randomisation.  Every environment is a robot of its own for the whole run: its sliding friction (every contact) is the model's times a scale
    # uniform in [friction_scale_min, friction_scale_max], its actuators' gain and bias are the model's times a scale uniform in [actuator_scale_min,
    # actuator_scale_max] (force and control ranges stay), and `added_mass_body` (a body name of the model; "": body 1, the first root) carries a point
    # payload uniform in [added_mass_min, added_mass_max] kg at its centre of mass.  Drawn once per environment from (training.seed, rank,
    # environment); in training, in `evaluate` - min = max asks "does this policy still stand at friction 0.3?" - and in `HumanoidEnv` / the `env` rollout.
    # All six at their defaults: off, nothing changes.  min > max or a negative scale: ValueError.
    friction_scale_min: float = field(default=1.0)
    friction_scale_max: float = field(default=1.0)
    actuator_scale_min: float = field(default=1.0)
    actuator_scale_max: float = field(default=1.0)
    added_mass_min: float = field(default=0.0)
    added_mass_max: float = field(default=0.0)
    added_mass_body: str = field(default="")
    # Extension (absent upstream; legged_gym `add_noise` / `noise_scale_vec`, MuJoCo Playground `noise_config`): sensor noise.  Above 0, every observation the
    # policy reads - the reset's included - is the simulator's plus U(-s_j, s_j) per column, s_j = obs_noise_level x the scale of the column's group in the
    # layout `qpos | qvel | cinert[1:] | cvel[1:] | qfrc_actuator` (without c-values: `qpos | qvel | qfrc_actuator`); the state itself stays exact (DESIGN.md
    # 3.12).  The group defaults are conventions, not measurements: legged_gym's and Playground's joint-position (0.01), angular-velocity (0.2) and
    # linear-velocity (0.1) scales; computed quantities (cinert, qfrc_actuator) default to 0.  A free joint's quaternion columns of qpos are perturbed like
    # any other column and not renormalised.  In training, in `evaluate` (under `deterministic` too) and in `HumanoidEnv`.  0: off, nothing changes.
    # A negative level or scale: ValueError.
    obs_noise_level: float = field(default=0.0)
    obs_noise_qpos: float = field(default=0.01)
    obs_noise_qvel: float = field(default=0.2)
    obs_noise_cinert: float = field(default=0.0)
    obs_noise_cvel: float = field(default=0.1)
    obs_noise_qfrc: float = field(default=0.0)
    # Extension (absent upstream; MuJoCo Playground's action latency, Isaac Lab `ActionDelay`): actuation latency.  Every environment has, for the whole run,
    # a latency of its own drawn in action_delay_min .. action_delay_max env steps (whatever n_frames is; at most 16): the actuators get the action the
    # policy computed that many steps ago in the same episode, zeros on an episode's first steps.  PPO's ratio keeps the policy's own
    # action; the reward's control cost sees the applied one.  In training, in `evaluate` and in `HumanoidEnv`.  0 / 0: off, nothing changes.
    # min < 0, min > max or max > 16: ValueError.
    action_delay_min: int = field(default=0)
    action_delay_max: int = field(default=0)


@dataclass
class VisualizationConfig:
    camera_name: str = field(default=MISSING)
    width: int = field(default=640)
    height: int = field(default=480)
    render_every: int = field(default=1)
    max_steps: int = field(default=1000)
    video_length: float = field(default=5.0)
    num_episodes: int = field(default=20)
    video_save_path: str = field(default="episode.mp4")


@dataclass
class RewardConfig:
    termination_height: float = field(default=-0.2)
    height_min_z: float = field(default=-0.2)
    height_max_z: float = field(default=2.0)
    is_healthy_reward: float = field(default=5)
    original_pos_reward_exp_coefficient: float = field(default=2)
    original_pos_reward_subtraction_factor: float = field(default=0.2)
    original_pos_reward_max_diff_norm: float = field(default=0.5)
    ctrl_cost_coefficient: float = field(default=0.1)
    weights_ctrl_cost: float = field(default=0.1)
    weights_original_pos_reward: float = field(default=4)
    weights_is_healthy: float = field(default=1)
    weights_velocity: float = field(default=1.25)


@dataclass
class ModelConfig:
    hidden_size: int = field(default=256)
    num_layers: int = field(default=2)
    use_tanh: bool = field(default=True)


@dataclass
class OptimizerConfig:
    lr: float = field(default=3e-4)
    max_grad_norm: float = field(default=0.5)


@dataclass
class ReinforcementLearningConfig:
    num_env_steps: int = field(default=10)
    gamma: float = field(default=0.99)
    gae_lambda: float = field(default=0.95)
    clip_eps: float = field(default=0.2)
    ent_coef: float = field(default=0.0)
    vf_coef: float = field(default=0.5)


@dataclass
class TrainingConfig:
    lr: float = field(default=3e-4)
    seed: int = field(default=1337)
    num_envs: int = field(default=2048)
    total_timesteps: int = field(default=1_000_000_000)
    num_minibatches: int = field(default=32)
    num_steps: int = field(default=10)
    update_epochs: int = field(default=4)
    anneal_lr: bool = field(default=True)
    model_save_path: str = field(default="trained_model.pkl")
    # Extension: MLP GEMM arithmetic. "f32" = exact f32 MFMA; "bf16" = bf16-in /
    # f32-accumulate MFMA (BASELINE config 4).  GAE and Adam are always f32.
    mlp_dtype: str = field(default="f32")
    rng_impl: str = field(default="philox")  # "philox": the engine's own streams; "threefry": jax.random-compatible streams following the reference's key plumbing (minppo_amd/jaxrng.py)
    # Extension (absent upstream): full-state checkpoints.  `checkpoint_path` is written every
    # `checkpoint_every` updates (0 = only at the end, "" = never); `resume_from` restores parameters, Adam moments,
    # step counters (LR schedule + RNG stream position), environment states and episode metrics before training.
    # Extension: `TrainOutput.metrics` in the REFERENCE's shape (train.py:283,287-289: the six `EnvMetrics` fields of every step of
    # every update, [num_updates, T, N] each) instead of the per-update device-side reductions.  Small runs only: every update then
    # synchronises and copies its [T, N] reward / done arrays out; refused above 1 GiB of history.
    keep_metrics_history: bool = field(default=False)
    # Extension (absent upstream; Brax `normalize_observations`, gym `NormalizeObservation`): running mean / standard deviation per observation
    # column, collected from the rollout's own rows, applied in place before the network sees them.  `obs_norm_clip` clamps the
    # normalised value to [-clip, clip] (0 = no clamp); `obs_norm_eps` is added to the variance.  Off: nothing changes.  Any number of ranks:
    # the statistics are those of all ranks' rows, bit-identical on every rank.
    normalize_observations: bool = field(default=False)
    obs_norm_clip: float = field(default=10.0)
    obs_norm_eps: float = field(default=1e-8)
    # Extension (absent upstream; gym `NormalizeReward`, SB3 `VecNormalize(norm_reward=True)`, Brax `reward_scaling`): the rewards GAE reads are divided
    # by the running standard deviation of the discounted return, collected on the device from the rollout's own rewards.  Scaled, never
    # centred; the scale is frozen within an update.  `reward_norm_clip` clamps the scaled reward to [-clip, clip] (0 = no clamp); `reward_norm_eps` is
    # added to the variance.  Metrics and `evaluate` report raw returns.  Off: nothing changes.  Any number of ranks, as above.
    normalize_rewards: bool = field(default=False)
    reward_norm_clip: float = field(default=10.0)
    reward_norm_eps: float = field(default=1e-8)
    checkpoint_path: str = field(default="")
    checkpoint_every: int = field(default=0)
    resume_from: str = field(default="")


@dataclass
class InferenceConfig:
    model_path: str = field(default=MISSING)


@dataclass
class EvaluationConfig:
    # Extension (absent upstream, whose `infer` is a stub): `minppo evaluate` / `minppo_amd.evaluate.evaluate` run the model file
    # `inference.model_path` for `num_steps` steps of `num_envs` environments (the reference has no time limit - env.py:238-242 - so the
    # horizon is fixed here) under the mean action (`deterministic`) or a sample; seed: `training.seed`; frames per step, reset noise and
    # the reward window: `environment` / `reward`.  `record_envs` > 0 keeps the joint trajectory of the first that many environments,
    # `trajectory_path` writes it as an .npz (qpos, qvel, action, reward, done, dt, n_frames).
    num_envs: int = field(default=256)
    num_steps: int = field(default=1000)
    deterministic: bool = field(default=True)
    record_envs: int = field(default=0)
    trajectory_path: str = field(default="")
    # `video_path` renders recorded environment 0's trajectory (camera and image size: `visualization`) and writes it as a video
    # (.npz / .avi / .mp4: minppo_amd.render.write_video) - train, then watch it.  Needs record_envs >= 1.
    video_path: str = field(default="")


@dataclass
class Config:
    kscale_id: str = field(default=MISSING)
    environment: EnvironmentConfig = field(default_factory=EnvironmentConfig)
    visualization: VisualizationConfig = field(default_factory=VisualizationConfig)
    reward: RewardConfig = field(default_factory=RewardConfig)
    model: ModelConfig = field(default_factory=ModelConfig)
    opt: OptimizerConfig = field(default_factory=OptimizerConfig)
    rl: ReinforcementLearningConfig = field(default_factory=ReinforcementLearningConfig)
    training: TrainingConfig = field(default_factory=TrainingConfig)
    inference: InferenceConfig = field(default_factory=InferenceConfig)
    evaluation: EvaluationConfig = field(default_factory=EvaluationConfig)
    debug: bool = field(default=True)


# ---------------------------------------------------------------------------
# merge machinery (dataclass <- nested dict <- dot-list)
# ---------------------------------------------------------------------------


def _coerce(value: Any, typ: Any, path: str) -> Any:
    """Converts a YAML / dot-list scalar to the declared field type."""
    if isinstance(value, _Missing):
        return value
    if typ in (int, "int"):
        if isinstance(value, bool):
            raise ValueError(f"{path}: expected int, got bool")
        if isinstance(value, float):
            if value != int(value):
                raise ValueError(f"{path}: expected int, got {value!r}")
            return int(value)
        if isinstance(value, str):
            return int(float(value)) if ("e" in value.lower() or "." in value) else int(value.replace("_", ""))
        return int(value)
    if typ in (float, "float"):
        return float(value)
    if typ in (bool, "bool"):
        if isinstance(value, str):
            low = value.strip().lower()
            if low in ("true", "1", "yes", "on"):
                return True
            if low in ("false", "0", "no", "off"):
                return False
            raise ValueError(f"{path}: expected bool, got {value!r}")
        return bool(value)
    if typ in (str, "str"):
        return str(value)
    return value


def _merge_into(obj: Any, upd: dict, prefix: str = "") -> None:
    if not isinstance(upd, dict):
        raise ValueError(f"{prefix or '<root>'}: expected a mapping, got {type(upd).__name__}")
    known = {f.name: f for f in fields(obj)}
    for key, val in upd.items():
        path = f"{prefix}{key}"
        if key not in known:
            raise ValueError(f"Key '{path}' is not in the config schema")
        cur = getattr(obj, key)
        if is_dataclass(cur):
            _merge_into(cur, val if val is not None else {}, path + ".")
        else:
            setattr(obj, key, _coerce(val, known[key].type, path))


def _dotlist_to_dict(items: Sequence[str]) -> dict:
    out: dict = {}
    for item in items:
        if "=" not in item:
            raise ValueError(f"Override '{item}' is not of the form key.path=value")
        key, raw = item.split("=", 1)
        val = yaml.safe_load(raw) if raw != "" else ""
        node = out
        parts = key.strip().split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
            if not isinstance(node, dict):
                raise ValueError(f"Override '{item}' conflicts with an earlier scalar override")
        node[parts[-1]] = val
    return out


def to_dict(cfg: Any) -> dict:
    out = {}
    for f in fields(cfg):
        v = getattr(cfg, f.name)
        out[f.name] = to_dict(v) if is_dataclass(v) else ("???" if isinstance(v, _Missing) else v)
    return out


def to_yaml(cfg: Any) -> str:
    return yaml.safe_dump(to_dict(cfg), sort_keys=False)


def require(value: Any, name: str) -> Any:
    """Returns `value`, raising if it is still MISSING (OmegaConf raises on access)."""
    if isinstance(value, _Missing):
        raise MissingMandatoryValue(f"Missing mandatory value: {name}")
    return value


def make_config(yaml_dict: dict | None = None, overrides: Sequence[str] = ()) -> Config:
    cfg = Config()
    if yaml_dict:
        _merge_into(cfg, yaml_dict)
    if overrides:
        _merge_into(cfg, _dotlist_to_dict(overrides))
    if not cfg.environment.reset_noise_scale >= 0.0:
        raise ValueError(f"environment.reset_noise_scale = {cfg.environment.reset_noise_scale!r}: the half-width of the reset noise cannot be negative")
    env = cfg.environment
    if not env.push_force >= 0.0:
        raise ValueError(f"environment.push_force = {env.push_force!r}: the size of the random pushes cannot be negative")
    if env.push_force > 0.0 and not (env.push_interval >= 1 and 1 <= env.push_duration <= env.push_interval):
        raise ValueError(f"environment.push_interval = {env.push_interval!r} / push_duration = {env.push_duration!r}: the interval is at least one env step and "
                         "the duration lies in 1 .. push_interval")
    if not env.episode_length >= 0:
        raise ValueError(f"environment.episode_length = {env.episode_length!r}: the time limit is a number of env steps (0: no limit) and cannot be negative")
    for what in ("friction_scale", "actuator_scale", "added_mass"):
        lo, hi = getattr(env, what + "_min"), getattr(env, what + "_max")
        if not lo <= hi:
            raise ValueError(f"environment.{what}_min = {lo!r} > environment.{what}_max = {hi!r}: the range of the domain randomisation is empty")
        if what != "added_mass" and not lo >= 0.0:
            raise ValueError(f"environment.{what}_min = {lo!r}: a scale of the domain randomisation cannot be negative")
    for key in ("obs_noise_level", "obs_noise_qpos", "obs_noise_qvel", "obs_noise_cinert", "obs_noise_cvel", "obs_noise_qfrc"):
        if not getattr(env, key) >= 0.0:
            raise ValueError(f"environment.{key} = {getattr(env, key)!r}: a half-width of the sensor noise cannot be negative")
    if not 0 <= env.action_delay_min <= env.action_delay_max <= 16:
        raise ValueError(f"environment.action_delay_min = {env.action_delay_min!r} / action_delay_max = {env.action_delay_max!r}: the latency is a number of env "
                         "steps with 0 <= min <= max <= 16")
    for key in ("obs_norm_clip", "obs_norm_eps", "reward_norm_clip", "reward_norm_eps"):
        if not getattr(cfg.training, key) >= 0.0:
            raise ValueError(f"training.{key} = {getattr(cfg.training, key)!r} cannot be negative")
    return cfg


def load_config_from_cli(args: Sequence[str] | None = None) -> Config:
    """Same contract as the reference's `load_config_from_cli` (`minppo/config.py:106-127`)."""
    if args is None:
        args = sys.argv[1:]
    if len(args) < 1:
        raise ValueError("Usage: <config_name_or_path> (<additional_args> ...)")
    path, *other_args = args

    if Path(path).exists():
        with open(path, "r", encoding="utf-8") as f:
            raw = yaml.safe_load(f) or {}
    elif (config_path := CONFIG_ROOT_DIR / f"{path}.yaml").exists():
        with open(config_path, "r", encoding="utf-8") as f:
            raw = yaml.safe_load(f) or {}
    else:
        raise ValueError(f"Config file not found: {path}")

    cfg = make_config(raw, other_args)
    logger.info("Loaded config: %s", to_yaml(cfg))
    return cfg


def replace(cfg: Any, **changes: Any) -> Any:
    return dataclasses.replace(cfg, **changes)
