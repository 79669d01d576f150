"""Definition of the humanoid environment — MI355X-native.

Keeps the surface of the reference's `minppo/env.py` (`HumanoidEnv(config)` with `reset`, `step`, `compute_reward`,
`is_done`, `get_obs`, `initial_qpos`, `actuator_ctrlrange`, `reward_config`, `observation_size`, `action_size`, `dt`;
`EnvState` / `EnvMetrics` records; `load_mjcf_model`), batched over environments: where the reference vmaps a
single-env function (`train.py:136,140`), every method here takes and returns `[N, ...]` torch CUDA tensors and runs the
cooperative rigid-body kernel (`csrc/k_physics.hip`) through the C ABI (`mppo_env_reset` / `mppo_env_step`).

`reset_noise_scale` is 0.0 in the reference (`env.py:87`): its reset is deterministic and its step keys draw noise of width
zero (`env.py:117-119`), so at scale 0 the `rng` arguments are accepted and ignored.  Above 0 (the attribute
assigned as in any Brax humanoid, or `environment.reset_noise_scale`) they are the reference's keys: `reset(rng, num_envs)` takes an
int seed or a `uint32[2]` key and splits it over the environments (`train.py:135`), `step(es, action, rng)` takes a `uint32[2]` key or
the `[N, 2]` per-environment keys the reference passes (`train.py:164-165`), and an environment that is reset starts from
`qpos0 + U(-s, s)`, `qvel = U(-s, s)` (`env.py:115-121`) in the conventions of `minppo_amd/jaxrng.py` (`mppo_env_reinit`).
`render(states, camera, width, height)` is Brax's `env.render` with the engine's own ray caster behind it (minppo_amd/render.py), and `main` is
the reference's debug viewer (`env.py:264-333`): a random-action rollout of one environment, rendered and written as a video.
"""

from __future__ import annotations

import ctypes as C
import logging
from typing import Any, NamedTuple, Optional, Sequence

import numpy as np

from minppo_amd import _native as nat
from minppo_amd.config import Config, load_config_from_cli, require
from minppo_amd.model import CompiledModel, load_model
from minppo_amd.train import action_delay_cfg, domain_body_id, domain_cfg, obs_noise_scales, push_body_id, push_cfg, resolve_model, reward_cfg

logger = logging.getLogger(__name__)


def load_mjcf_model(kscale_id: str) -> CompiledModel:
    """Stands where the reference downloads and patches the MJCF (`env.py:27-50`): resolves the id (or a built-in
    model name / MJCF path) through the local robot table (minppo_amd/model.py)."""
    return load_model(kscale_id)


class EnvMetrics(NamedTuple):
    episode_returns: Any
    episode_lengths: Any
    returned_episode_returns: Any
    returned_episode_lengths: Any
    timestep: Any
    returned_episode: Any


class _EnvStateFields(NamedTuple):
    pipeline_state: Any  # [N, rec_dim] float32 record (layout: include/minppo_hip.h)
    obs: Any
    reward: Any
    done: Any
    metrics: EnvMetrics
    truncation: Any = None  # extension (Brax: `state.info["truncation"]`): bool [N], the environments `environment.episode_length` cut at this step (a subset of `done`); None without a limit


class EnvState(_EnvStateFields):
    """The six fields above - as a tuple it is what it always was - plus the optional trailing `action_history` (extension): float32 [D, N, A], the ring of the
    policy's past actions under `environment.action_delay_max` = D > 0 (slot metrics.timestep mod D holds that step's action); None without a latency.  It is an
    attribute beside the tuple's fields, not a seventh element: `len`, unpacking and `_replace` see six (`_replace` returns a state without it)."""

    action_history: Any = None

    def __new__(cls, pipeline_state, obs, reward, done, metrics, truncation=None, action_history=None):
        self = super().__new__(cls, pipeline_state, obs, reward, done, metrics, truncation)
        self.action_history = action_history
        return self


class HumanoidEnv:
    """Batched humanoid environment on one GPU."""

    reset_noise_scale: float = 0.0

    def __init__(self, config: Config, *, lib: Optional[nat.Lib] = None, device: Any = "cuda:0") -> None:
        import torch

        self.torch = torch
        self.lib = lib if lib is not None else nat.load()
        self.device = torch.device(device)
        self._include_c_vals = config.environment.include_c_vals
        self._kscale_id = config.kscale_id
        self.cm = resolve_model(config)
        # the body `step(..., xfrc=)` acts on: the name is resolved - and an unknown one refused, before anything is opened - even at push_force = 0
        # (an explicit wrench needs no random draw)
        self._push_body = push_body_id(config, self.cm, always=True)
        self._n_frames = config.environment.n_frames
        self._blob_host = np.frombuffer(self.cm.to_blob(self._include_c_vals), np.uint8).copy()
        self._blob_dev = torch.from_numpy(self._blob_host.copy()).to(self.device)
        self._model = C.c_void_p()
        with torch.cuda.device(self.device):
            self.lib.model_open(self._blob_host.ctypes.data, self._blob_host.size, self._blob_dev.data_ptr(), C.byref(self._model))
        if config.environment.jit_kernel:
            from minppo_amd import jit

            with torch.cuda.device(self.device):
                jit.specialize(self.lib, self._model, self.cm)
        self.dims = nat.ModelDims()
        self.lib.model_get_dims(self._model, C.byref(self.dims))
        self._action_size = self.cm.nu
        self.initial_qpos = torch.tensor(self.cm.t["qpos0"], dtype=torch.float32, device=self.device)
        self.reward_config = config.reward
        self._rc = reward_cfg(config)
        # "Currently unused" in the reference as well (env.py:107-113)
        self.actuator_ctrlrange = torch.tensor(self.cm.t["act_ctrlrange"], dtype=torch.float32, device=self.device)
        self._reset_rec = torch.zeros(self.dims.rec_dim, dtype=torch.float32, device=self.device)
        # `environment.reset_noise_scale` sets the attribute unless it was assigned directly (on the class, or on the instance later)
        if type(self).reset_noise_scale == 0.0 and config.environment.reset_noise_scale > 0:
            self.reset_noise_scale = float(config.environment.reset_noise_scale)
        # random pushes (`environment.push_*`): what `push_wrench` draws (None: push_force = 0)
        self._push = push_cfg(config, self.cm, config.training.seed)
        # the episode time limit (`environment.episode_length`; 0: none): applied behind every step, every episode cut at the same length (no stagger)
        self._limit = nat.TimeLimitCfg(length=int(config.environment.episode_length), stagger=0, rank=0, reserved=0, seed=int(config.training.seed) & 0xFFFFFFFFFFFFFFFF)
        # domain randomisation (`environment.friction_scale_* / actuator_scale_* / added_mass_*`): what `domain_params` draws (None: every range at its default);
        # the payload's body is resolved whatever the ranges are - `reset(..., domain=)` takes an explicit table.  `_domain`: the table of the last reset
        self._domain_cfg = domain_cfg(config, self.cm, config.training.seed)
        self._domain_body = domain_body_id(config, self.cm, always=True)
        self._domain = None
        # sensor noise (`environment.obs_noise_*`): the per-column half-widths as the [OP] device table the kernel reads (None: off); rank 0, seed `training.seed`,
        # the step index metrics.timestep[0] (0 for `reset`).  Actuation latency (`environment.action_delay_min / _max`): `_delays` is the table of the last reset
        sig = obs_noise_scales(config, self.cm)
        self._obs_noise = None
        if sig is not None:
            table = np.zeros(self.dims.obs_pad, np.float32)
            table[:sig.size] = sig
            self._obs_noise = torch.from_numpy(table).to(self.device)
        self._noise_cfg = nat.ObsNoiseCfg(seed=int(config.training.seed) & 0xFFFFFFFFFFFFFFFF, rank=0, reserved=0)
        self._delay_cfg = action_delay_cfg(config, config.training.seed)
        self._delays = None
        self._have_reset = False
        self._camera_name = config.visualization.camera_name
        self._renderer = None

    # -- PipelineEnv attributes ------------------------------------------------
    @property
    def observation_size(self) -> int:
        return self.dims.obs_dim

    @property
    def action_size(self) -> int:
        return self._action_size

    @property
    def dt(self) -> float:
        return float(self.dims.timestep) * self._n_frames

    def _stream(self) -> int:
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _metrics(self, N: int) -> EnvMetrics:
        t = self.torch
        z = lambda dt: t.zeros(N, dtype=dt, device=self.device)
        return EnvMetrics(z(t.float32), z(t.int32), z(t.float32), z(t.int32), z(t.int32), z(t.uint8))

    @staticmethod
    def _mstruct(m: EnvMetrics) -> nat.EnvMetrics:
        return nat.EnvMetrics(*[x.data_ptr() for x in m])

    def _noise_keys(self, rng: Any, N: int, what: str):
        """-> (rng_impl of mppo_env_reinit, device tensor of the key words) for a seed, a uint32[2] key or [N, 2] per-environment keys"""
        t = self.torch
        scale = float(self.reset_noise_scale)
        if scale < 0:
            raise ValueError(f"reset_noise_scale = {scale!r}: the half-width of the reset noise cannot be negative")
        if rng is None:
            raise ValueError(f"{what}: reset_noise_scale = {scale} needs `rng` (an int seed or a uint32[2] key" + (", or [N, 2] per-environment keys)" if what == "step" else ")"))
        if isinstance(rng, (int, np.integer)):
            from minppo_amd import jaxrng

            key = jaxrng.prng_key(int(rng))
        else:
            key = (rng.detach().cpu().numpy() if hasattr(rng, "detach") else np.asarray(rng)).astype(np.uint32)
        if key.shape == (2,):
            impl = 1
        elif what == "step" and key.shape == (N, 2):
            impl = 2
        else:
            raise ValueError(f"{what}: rng must be an int seed or a uint32[2] key" + (f" or [{N}, 2] per-environment keys" if what == "step" else "") + f", got shape {key.shape}")
        return impl, t.from_numpy(np.ascontiguousarray(key).view(np.int32)).to(self.device)

    # -- env.py:124-145 ---------------------------------------------------------
    def reset(self, rng: Any = None, num_envs: int = 1, *, domain: Any = None) -> EnvState:
        """`domain` (extension; Brax `domain_randomize`'s vmapped model): [N, 4] rows (friction_scale, actuator_scale, added_mass, 0) - environment n is then
        the robot whose sliding friction, actuator gain / bias and `environment.added_mass_body`'s mass are replaced by its row, in this reset and in every
        `step` until the next reset.  None: the table `domain_params(num_envs)` draws when the configuration's ranges are on, else no randomisation.
        The table belongs to this object, not to the returned `EnvState`: `step` uses the table of the LAST reset, so an `EnvState` kept from before a later
        reset is stepped on the later reset's robots (only a different number of environments is refused) - step the states of one reset at a time."""
        t = self.torch
        N = int(num_envs)
        if domain is not None:
            domain = (domain if hasattr(domain, "data_ptr") else t.as_tensor(np.asarray(domain, np.float32))).to(device=self.device, dtype=t.float32).contiguous()
            if domain.shape != (N, 4):
                raise ValueError(f"domain must have shape ({N}, 4) - friction_scale, actuator_scale, added_mass, 0 per environment - got {tuple(domain.shape)}")
        elif self._domain_cfg is not None:
            domain = self.domain_params(N)
        self._domain = domain
        noise = self._noise_keys(rng, N, "reset") if self.reset_noise_scale != 0 else None  # (a missing key is refused before anything is launched)
        state = t.empty(N, self.dims.rec_dim, dtype=t.float32, device=self.device)
        obs = t.empty(N, self.dims.obs_pad, dtype=t.float32, device=self.device)
        reward, done = t.empty(N, dtype=t.float32, device=self.device), t.empty(N, dtype=t.uint8, device=self.device)
        m = self._metrics(N)
        ms = self._mstruct(m)
        if domain is not None:  # every robot's own reset (mppo_env_reset_domain: the reset kernel with the environment's row)
            self.lib.env_reset_domain(self._model, N, state.data_ptr(), self._reset_rec.data_ptr(), obs.data_ptr(), self.dims.obs_pad, reward.data_ptr(),
                                      done.data_ptr(), C.byref(ms), None, domain.data_ptr(), self._domain_body, 0.0, 0, 0, 0, None, None, 0, self._stream())
        else:
            self.lib.env_reset(self._model, N, state.data_ptr(), self._reset_rec.data_ptr(), obs.data_ptr(), self.dims.obs_pad, reward.data_ptr(),
                               done.data_ptr(), C.byref(ms), self._stream())
        if noise is not None:  # env.py:115-121: every environment from a state of its own, keyed by split(rng, num_envs) (train.py:135)
            impl, keys = noise
            if domain is not None:
                self.lib.env_reset_domain(self._model, N, state.data_ptr(), None, obs.data_ptr(), self.dims.obs_pad, None, None, None, None, domain.data_ptr(),
                                          self._domain_body, float(self.reset_noise_scale), impl, 0, 0, keys.data_ptr(), None, 0, self._stream())
            else:
                self.lib.env_reinit(self._model, N, state.data_ptr(), obs.data_ptr(), self.dims.obs_pad, 0, float(self.reset_noise_scale), impl, 0, 0, keys.data_ptr(), 0, 0,
                                    self._stream())
            self._noise_keep = keys  # (lives until the next call: the launch reads it; same-stream allocations are reused in stream order)
        if self._obs_noise is not None:  # the policy's first observation is a noisy one too (step 0 of the noise's stream); the state stays exact
            self.lib.obs_noise_apply(C.byref(self._noise_cfg), N, self.observation_size, obs.data_ptr(), self.dims.obs_pad, self._obs_noise.data_ptr(), None, 0, 0,
                                     self._stream())
        hist = None
        if self._delay_cfg is not None:  # every environment's latency for its steps until the next reset, and an empty ring
            self._delays = self.action_delays(N)
            hist = t.zeros(self._delay_cfg.max, N, self._action_size, dtype=t.float32, device=self.device)
        self._have_reset = True
        return EnvState(state, obs[:, :self.observation_size], reward, done.bool(), m, None, hist)

    # -- env.py:148-196 -----------------------------------------------------------
    def step(self, env_state: EnvState, action: Any, rng: Any = None, *, xfrc: Any = None) -> EnvState:
        """`xfrc` (extension; Brax: `pipeline_state.xfrc_applied`): [N, 6] external wrench per environment - force, then torque, world axes, at the
        centre of mass of the body `environment.push_body` (default: body 1, the first root; read whatever `environment.push_force` is) - held for the
        whole step (`mppo_env_step_xfrc`).  With `environment.episode_length` > 0 an environment whose episode reaches that many steps is truncated
        (`mppo_env_time_limit`): `done` and the metrics as for an ended episode, its state and observation those of the reset (or, under reset noise,
        of a fresh noisy one), and `truncation` says which environments those were."""
        t = self.torch
        if not self._have_reset:
            self.reset(num_envs=1)
        state = env_state.pipeline_state.clone()
        N = state.shape[0]
        noise = self._noise_keys(rng, N, "step") if self.reset_noise_scale != 0 else None
        action = action.to(device=self.device, dtype=t.float32).contiguous()
        if action.shape != (N, self._action_size):
            raise ValueError(f"action must have shape ({N}, {self._action_size}), got {tuple(action.shape)}")
        obs = t.empty(N, self.dims.obs_pad, dtype=t.float32, device=self.device)
        reward, done = t.empty(N, dtype=t.float32, device=self.device), t.empty(N, dtype=t.uint8, device=self.device)
        m = EnvMetrics(*[x.clone() if x.dtype != t.bool else x.to(t.uint8) for x in env_state.metrics])
        ms = self._mstruct(m)
        dom = self._domain
        if dom is not None and dom.shape[0] != N:
            raise ValueError(f"step: {N} environments, but the last reset randomised {dom.shape[0]} - reset(num_envs={N}) first")
        hist = None
        if self._delay_cfg is not None:  # actuation latency: the step is given the action of the environment's latency ago (mppo_action_delay_apply, on the metrics as they stand before the step)
            if env_state.action_history is None or self._delays is None or self._delays.shape[0] != N:
                raise ValueError("step: environment.action_delay_max > 0 needs the EnvState of a reset() of this environment (its action_history and latency table)")
            hist = env_state.action_history.clone()
            applied = t.empty(N, self._action_size, dtype=t.float32, device=self.device)
            self.lib.action_delay_apply(C.byref(self._delay_cfg), N, self._action_size, self._delays.data_ptr(), m.timestep.data_ptr(), m.episode_lengths.data_ptr(),
                                        action.data_ptr(), self._action_size, hist.data_ptr(), applied.data_ptr(), self._action_size, self._stream())
            action = applied
        if xfrc is not None:
            xfrc = (xfrc if hasattr(xfrc, "data_ptr") else t.as_tensor(np.asarray(xfrc, np.float32))).to(device=self.device, dtype=t.float32).contiguous()
            if xfrc.shape != (N, 6):
                raise ValueError(f"xfrc must have shape ({N}, 6) - force, then torque, per environment - got {tuple(xfrc.shape)}")
            self._xfrc_keep = xfrc  # (lives until the next call: the launch reads it)
        if dom is not None:  # the randomised step (mppo_env_step_domain), with or without a wrench
            self.lib.env_step_domain(self._model, N, self._n_frames, C.byref(self._rc), state.data_ptr(), self._reset_rec.data_ptr(), action.data_ptr(),
                                     self._action_size, obs.data_ptr(), self.dims.obs_pad, reward.data_ptr(), done.data_ptr(), C.byref(ms), self._push_body,
                                     None if xfrc is None else xfrc.data_ptr(), dom.data_ptr(), self._domain_body, self._stream())
        elif xfrc is not None:
            self.lib.env_step_xfrc(self._model, N, self._n_frames, C.byref(self._rc), state.data_ptr(), self._reset_rec.data_ptr(), action.data_ptr(),
                                   self._action_size, obs.data_ptr(), self.dims.obs_pad, reward.data_ptr(), done.data_ptr(), C.byref(ms), self._push_body,
                                   xfrc.data_ptr(), self._stream())
        else:
            self.lib.env_step(self._model, N, self._n_frames, C.byref(self._rc), state.data_ptr(), self._reset_rec.data_ptr(), action.data_ptr(),
                              self._action_size, obs.data_ptr(), self.dims.obs_pad, reward.data_ptr(), done.data_ptr(), C.byref(ms), self._stream())
        truncated = None
        if self._limit.length > 0:  # in front of the masked reinit: its mask `done` then includes the truncated environments
            truncated = t.empty(N, dtype=t.uint8, device=self.device)
            self.lib.env_time_limit(self._model, N, C.byref(self._limit), state.data_ptr(), self._reset_rec.data_ptr(), obs.data_ptr(), self.dims.obs_pad,
                                    done.data_ptr(), truncated.data_ptr(), C.byref(ms), self._stream())
        if dom is not None:  # every restart through the reset kernel with the environment's own row: the one shared reset record is another robot's
            impl, keys = noise if noise is not None else (0, None)
            self.lib.env_reset_domain(self._model, N, state.data_ptr(), None, obs.data_ptr(), self.dims.obs_pad, None, None, None, done.data_ptr(), dom.data_ptr(),
                                      self._domain_body, float(self.reset_noise_scale) if noise is not None else 0.0, impl, 0, 0,
                                      None if keys is None else keys.data_ptr(), None, 0, self._stream())
            self._noise_keep = keys
        elif noise is not None:  # env.py:166,179-180: the environments that ended restart from `_get_reset_state(rng)`, not from the constant record
            impl, keys = noise
            self.lib.env_reinit(self._model, N, state.data_ptr(), obs.data_ptr(), self.dims.obs_pad, done.data_ptr(), float(self.reset_noise_scale), impl, 0, 0,
                                keys.data_ptr(), 0, 0, self._stream())
            self._noise_keep = keys
        if self._obs_noise is not None:  # behind the restarts, so their rows are noisy too; the step index is environment 0's timestep after the step, read on the device
            self.lib.obs_noise_apply(C.byref(self._noise_cfg), N, self.observation_size, obs.data_ptr(), self.dims.obs_pad, self._obs_noise.data_ptr(),
                                     m.timestep.data_ptr(), 1, 0, self._stream())
        return EnvState(state, obs[:, :self.observation_size], reward, done.bool(), m, None if truncated is None else truncated.bool(), hist)

    def push_wrench(self, step: int, num_envs: int, seed: Optional[int] = None) -> Any:
        """The wrench [num_envs, 6] the random pushes of `environment.push_force / push_interval / push_duration` put on the environments at env step
        `step` (`mppo_push_fill`; rank 0; seed: `training.seed`), to be handed to `step(..., xfrc=)`; `jaxrng.push_wrench_philox` is its host statement."""
        if self._push is None:
            raise ValueError("push_wrench: environment.push_force is 0 - there are no pushes to draw")
        t = self.torch
        p = nat.PushCfg.from_buffer_copy(self._push)
        if seed is not None:
            p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        out = t.empty(int(num_envs), 6, dtype=t.float32, device=self.device)
        self.lib.push_fill(C.byref(p), int(num_envs), None, 0, int(step) & 0x7FFFFFFF, out.data_ptr(), self._stream())
        return out

    def domain_params(self, num_envs: int, seed: Optional[int] = None) -> Any:
        """The table [num_envs, 4] of the domain randomisation - rows (friction_scale, actuator_scale, added_mass, 0) - that `reset(num_envs=)` draws and
        keeps for its steps (`mppo_domain_fill`; rank 0; seed: `training.seed`); `jaxrng.domain_params_philox` is its host statement."""
        if self._domain_cfg is None:
            raise ValueError("domain_params: every environment.friction_scale_* / actuator_scale_* / added_mass_* key is at its default - there is nothing to draw")
        t = self.torch
        p = nat.DomainCfg.from_buffer_copy(self._domain_cfg)
        if seed is not None:
            p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        out = t.empty(int(num_envs), 4, dtype=t.float32, device=self.device)
        self.lib.domain_fill(C.byref(p), int(num_envs), out.data_ptr(), self._stream())
        return out

    def obs_noise_scales(self) -> np.ndarray:
        """The half-width of the sensor noise per observation column, float32 [O] (`environment.obs_noise_level` x the scale of the column's group; all zero
        when the noise is off); `jaxrng.obs_noise_philox(seed, 0, step, num_envs, scales)` is the noise of step `step` (0: `reset`, else metrics.timestep[0])."""
        if self._obs_noise is None:
            return np.zeros(self.observation_size, np.float32)
        return self._obs_noise[:self.observation_size].cpu().numpy()

    def action_delays(self, num_envs: int, seed: Optional[int] = None) -> Any:
        """The latency, in env steps, of each of `num_envs` environments - int32 [num_envs] - that `reset(num_envs=)` draws and keeps for its steps
        (`mppo_action_delay_fill`; rank 0; seed: `training.seed`); `jaxrng.action_delays_philox` is its host statement."""
        if self._delay_cfg is None:
            raise ValueError("action_delays: environment.action_delay_max is 0 - there is no latency to draw")
        t = self.torch
        p = nat.ActionDelayCfg.from_buffer_copy(self._delay_cfg)
        if seed is not None:
            p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        out = t.empty(int(num_envs), dtype=t.int32, device=self.device)
        self.lib.action_delay_fill(C.byref(p), int(num_envs), out.data_ptr(), self._stream())
        return out

    # -- env.py:245-261 / 238-242 / 199-235 on the state record (host-side views, for inspection) ------
    def get_obs(self, data: Any, action: Any = None) -> Any:
        return data[:, :self.observation_size]

    def is_done(self, state: Any) -> Any:
        z = state[:, 2]
        r = self.reward_config
        return ~((r.height_min_z < z) & (z < r.height_max_z))

    def compute_reward(self, state: Any, next_state: Any, action: Any) -> Any:
        t, r = self.torch, self.reward_config
        nq, nv, OP = self.cm.nq, self.cm.nv, self.dims.obs_pad
        p0 = t.linalg.norm(self.initial_qpos[None] - state[:, :nq], dim=-1)
        pos_r = t.exp(-r.original_pos_reward_exp_coefficient * p0) - r.original_pos_reward_subtraction_factor * t.clamp(p0, 0, r.original_pos_reward_max_diff_norm)
        z = state[:, 2]
        healthy = t.where(z < r.height_min_z, 0.0, 1.0)
        healthy = t.where(z > r.height_max_z, t.zeros_like(healthy), healthy)
        ctrl = -(action * action).sum(-1)
        vel = (next_state[:, OP + nv] - state[:, OP + nv]) / self.dt
        return r.weights_ctrl_cost * ctrl + r.weights_original_pos_reward * pos_r + r.weights_velocity * vel + r.weights_is_healthy * healthy

    # -- Brax's env.render(trajectory, camera, width, height) (what env.py:322-329 calls) ------------------------------------
    def render(self, states: Any, camera: Optional[str] = None, width: int = 640, height: int = 480, env_index: int = 0) -> np.ndarray:
        """Frames of a rollout, uint8 [F, H, W, 3], ray-cast on the device (minppo_amd/render.py).  `states`: a [F, nq] or [F, rec_dim]
        tensor / array (joint positions, or state records - qpos leads a record), a sequence of `EnvState`s, or a sequence of
        `pipeline_state` tensors [N, rec_dim]; of a batched state the environment `env_index` is drawn.  `camera=None`: the config's
        `visualization.camera_name`."""
        from minppo_amd.render import Renderer

        t = self.torch
        if camera is None:
            camera = require(self._camera_name, "visualization.camera_name")
        if isinstance(states, (list, tuple)):
            if not states:
                raise ValueError("render: no states")
            rows = []
            for s in states:
                ps = s.pipeline_state if isinstance(s, EnvState) else s
                ps = ps if hasattr(ps, "data_ptr") else t.as_tensor(np.asarray(ps, np.float32))
                if ps.ndim == 2:
                    if not 0 <= env_index < ps.shape[0]:
                        raise ValueError(f"render: env_index {env_index} of {ps.shape[0]} environments")
                    ps = ps[env_index]
                rows.append(ps.to(device=self.device, dtype=t.float32))
            q = t.stack(rows)
        else:
            q = states if hasattr(states, "data_ptr") else t.as_tensor(np.asarray(states, np.float32))
            q = q.to(device=self.device, dtype=t.float32)
        if q.ndim != 2 or q.shape[1] not in (self.cm.nq, self.dims.rec_dim):
            raise ValueError(f"render: states must be [F, {self.cm.nq}] joint positions or [F, {self.dims.rec_dim}] state records, got {tuple(q.shape)}")
        if self._renderer is None:  # (opened on the first render)
            self._renderer = Renderer(self.cm, lib=self.lib, device=self.device)
        return self._renderer.render(q, camera, width, height)

    def close(self) -> None:
        if getattr(self, "_renderer", None) is not None:
            self._renderer.close()
            self._renderer = None
        if getattr(self, "_model", None):
            self.lib.model_close(self._model)
            self._model = None


def main(args: Sequence[str] | None = None) -> None:
    """The reference's `minppo env` (`env.py:264-333`): runs `visualization.num_episodes` episodes of at most `max_steps` steps of one
    environment under actions drawn from U(0, 1), collects the states of the first `video_length * fps` steps (fps = int(1 / env.dt)),
    renders every `render_every`-th of them with `visualization.camera_name / width / height` and writes `video_save_path`.  As in the
    reference, the video's fps is NOT divided by `render_every`."""
    import sys

    import torch

    from minppo_amd.render import write_video

    logging.basicConfig(level=logging.INFO)
    config = load_config_from_cli(sys.argv[1:] if args is None else args)
    vis = config.visualization
    env = HumanoidEnv(config)
    try:
        logger.info("Initialized environment with action size %d", env.action_size)
        gen = torch.Generator(device="cpu").manual_seed(int(config.training.seed))
        fps = int(1 / env.dt)
        max_frames = int(vis.video_length * fps)
        rollout = []
        n_steps = 0  # (env steps so far, over all episodes: the pushes' step index - a push keeps running across a restart)
        for episode in range(int(vis.num_episodes)):
            seed = int(torch.randint(0, 2**31 - 1, (1,), generator=gen))
            es = env.reset(seed if env.reset_noise_scale != 0 else None, num_envs=1)
            total = 0.0
            pushed = config.environment.push_force > 0  # (random pushes: the rollout is shoved as a training environment is, so a push can be watched)
            for _ in range(int(vis.max_steps)):
                if len(rollout) < vis.video_length * fps:
                    rollout.append(es.pipeline_state[0].clone())
                action = torch.rand(1, env.action_size, generator=gen).to(env.device)
                step_seed = int(torch.randint(0, 2**31 - 1, (1,), generator=gen))
                es = env.step(es, action, step_seed if env.reset_noise_scale != 0 else None, xfrc=env.push_wrench(n_steps, 1) if pushed else None)
                n_steps += 1
                total += float(es.reward[0])
                if bool(es.done[0]):
                    break
            logger.info("Episode %d total reward: %f", episode + 1, total)
            if len(rollout) >= max_frames:
                break
        if not rollout:
            raise ValueError(f"visualization.video_length = {vis.video_length} and max_steps = {vis.max_steps} leave no frame to render")
        logger.info("Rendering video with %d frames at %d fps", len(rollout), fps)
        images = env.render(torch.stack(rollout[::max(1, int(vis.render_every))]), camera=vis.camera_name, width=vis.width, height=vis.height)
        write_video(vis.video_save_path, images, fps=fps)
        logger.info("Video saved to %s", vis.video_save_path)
    finally:
        env.close()


if __name__ == "__main__":
    main()
