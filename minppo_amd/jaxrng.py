"""JAX-stream-compatible random numbers without JAX.

The reference draws its randomness with `jax.random` on threefry2x32 keys (`minppo/train.py:110,142,158,163-164,252,258,285,303`).
This module restates, in NumPy, exactly the pieces the training loop uses, so that "identical seeds" can mean JAX seeds:

  prng_key(seed)                    jax.random.PRNGKey        -> uint32[2] = (seed >> 32, seed & 0xffffffff)
  split(key, num)                   jax.random.split          (threefry_split: threefry_2x32(key, iota(2 num)).reshape(num, 2))
  random_bits(key, n)               jax.random.bits / _random_bits (32-bit)
  uniform(key, n, lo, hi)           jax.random.uniform        (mantissa trick: bits >> 9 | 0x3f800000, minus 1)
  normal(key, n)                    jax.random.normal         (sqrt(2) erf_inv(uniform in (-1, 1)), XLA's float32 erf_inv polynomial)
  permutation(key, n)               jax.random.permutation    (ceil(3 ln n / ln(2^32 - 1)) rounds of a stable sort by fresh random bits)
  update_keys(rng, T, E)            the split tree of one `_update_step` (train.py:158,163,252)
  update_keys_step(rng, T, E)       the same, with the T step keys (train.py:163)
  reset_noise(key, N, nq, nv, s)    the noise of `_get_reset_state` for N environments keyed by split(key, N) (train.py:135,164; env.py:116-119)

Conventions are those of jax 0.4.3x with its defaults (`jax_default_prng_impl = threefry2x32`, `jax_threefry_partitionable = False`),
the versions the reference's un-pinned requirements resolved to in October 2024.  STATUS: written from the published algorithm and
checked against the Threefry-2x32-20 known-answer vectors of Random123 and against the few `jax.random` values that are common
knowledge (tests/test_jaxrng.py); JAX itself is not installed here, so bit-equality of long streams with a real JAX run has not
been measured.  The engine's device kernels (`mppo_threefry_*`, csrc/k_rng.hip) are tested bit for bit against this module.
"""

from __future__ import annotations

import math
from typing import Tuple

import numpy as np

_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
_PARITY = np.uint32(0x1BD11BDA)


def _rotl(x: np.ndarray, r: int) -> np.ndarray:
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def threefry2x32(key: Tuple[int, int], x0: np.ndarray, x1: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Threefry-2x32, 20 rounds (Salmon et al., SC'11), element-wise over the counter arrays."""
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    ks = (k0, k1, np.uint32(k0 ^ k1 ^ _PARITY))
    with np.errstate(over="ignore"):
        x0 = x0.astype(np.uint32) + ks[0]
        x1 = x1.astype(np.uint32) + ks[1]
        for i in range(5):
            for r in _ROT[i % 2]:
                x0 = x0 + x1
                x1 = _rotl(x1, r) ^ x0
            x0 = x0 + ks[(i + 1) % 3]
            x1 = x1 + ks[(i + 2) % 3] + np.uint32(i + 1)
    return x0, x1


def prng_key(seed: int) -> np.ndarray:
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.array([seed >> 32, seed & 0xFFFFFFFF], np.uint32)


def _threefry_counts(key, n: int) -> np.ndarray:
    """threefry_2x32(key, iota(n)): the counter array is split into halves (padded to even length), the cipher runs on the
    pairs (first half, second half) and the two output halves are concatenated."""
    half = (n + 1) // 2
    c = np.arange(2 * half, dtype=np.uint32)
    if n % 2:
        c[-1] = 0  # the padding word
    y0, y1 = threefry2x32((key[0], key[1]), c[:half], c[half:])
    return np.concatenate([y0, y1])[:n]


def split(key, num: int = 2) -> np.ndarray:
    return _threefry_counts(key, 2 * num).reshape(num, 2)


def random_bits(key, n: int) -> np.ndarray:
    return _threefry_counts(key, n)


def uniform(key, n: int, minval: float = 0.0, maxval: float = 1.0) -> np.ndarray:
    bits = random_bits(key, n)
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    lo, hi = np.float32(minval), np.float32(maxval)
    return np.maximum(lo, f * (hi - lo) + lo).astype(np.float32)


_ERFINV_LT = np.array([2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164, 0.246640727, 1.50140941], np.float32)
_ERFINV_GE = np.array([-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047, 1.00167406, 2.83297682], np.float32)


def erf_inv_f32(x: np.ndarray) -> np.ndarray:
    """XLA's float32 erf_inv (Giles' polynomial): w = -log1p(-x x); two branches at w = 5."""
    x = x.astype(np.float32)
    w = -np.log1p(-(x * x)).astype(np.float32)
    lt = w < np.float32(5.0)
    w = np.where(lt, w - np.float32(2.5), np.sqrt(w, dtype=np.float32) - np.float32(3.0)).astype(np.float32)
    p = np.where(lt, _ERFINV_LT[0], _ERFINV_GE[0]).astype(np.float32)
    for i in range(1, 9):
        p = (np.where(lt, _ERFINV_LT[i], _ERFINV_GE[i]).astype(np.float32) + p * w).astype(np.float32)
    out = (p * x).astype(np.float32)
    return np.where(np.abs(x) == np.float32(1.0), np.float32(np.inf) * x, out).astype(np.float32)


def normal(key, n: int) -> np.ndarray:
    lo = np.nextafter(np.float32(-1.0), np.float32(0.0))
    u = uniform(key, n, lo, 1.0)
    return (np.float32(math.sqrt(2.0)) * erf_inv_f32(u)).astype(np.float32)


def permutation_rounds(n: int) -> int:
    return int(math.ceil(3 * math.log(max(1, n)) / math.log(np.iinfo(np.uint32).max)))


def permutation(key, n: int) -> np.ndarray:
    x = np.arange(n, dtype=np.int32)
    key = np.asarray(key, np.uint32)
    for _ in range(permutation_rounds(n)):
        key, sub = split(key)
        x = x[np.argsort(random_bits(sub, n), kind="stable")]
    return x


def update_keys_step(rng, T: int, E: int, n_perm: int):
    """The split tree of one `_update_step` (reference train.py): per env step `rng, action_rng = split(rng)` (:158) and
    `rng, step_rng = split(rng)` (:163; the per-env keys split from it draw the reset noise, if there is any), per epoch
    `rng, _rng = split(rng)` (:252) followed by `_shuffle`'s `key, subkey = split(key)` per sort round.
    Returns (new rng, action keys [T,2], sort keys [E, rounds, 2], step keys [T,2])."""
    rng = np.asarray(rng, np.uint32)
    rounds = permutation_rounds(n_perm)
    act = np.zeros((T, 2), np.uint32)
    step = np.zeros((T, 2), np.uint32)
    for t in range(T):
        rng, act[t] = split(rng)
        rng, step[t] = split(rng)
    srt = np.zeros((E, rounds, 2), np.uint32)
    for e in range(E):
        rng, k = split(rng)
        for r in range(rounds):
            k, srt[e, r] = split(k)
    return rng, act, srt, step


def update_keys(rng, T: int, E: int, n_perm: int):
    """update_keys_step without the step keys: (new rng, action keys [T,2], sort keys [E, rounds, 2])."""
    return update_keys_step(rng, T, E, n_perm)[:3]


def reset_noise(key, num_envs: int, nq: int, nv: int, scale: float, env_keys=None):
    """The noise `_get_reset_state` (env.py:115-121) adds for each of `num_envs` environments under `reset_fn` / `step_fn`'s keys
    (train.py:135,164: `split(key, num_envs)`, or `env_keys` [N,2] given directly): `rng1, rng2 = split(key_n)`, qpos noise
    `uniform(rng1, (nq,), -s, s)`, qvel noise `uniform(rng2, (nv,), -s, s)` -> float32 [N, nq], [N, nv]."""
    keys = split(np.asarray(key, np.uint32), num_envs) if env_keys is None else np.asarray(env_keys, np.uint32).reshape(num_envs, 2)
    dq, dv = np.zeros((num_envs, nq), np.float32), np.zeros((num_envs, nv), np.float32)
    for n in range(num_envs):
        r1, r2 = split(keys[n])
        dq[n], dv[n] = uniform(r1, nq, -scale, scale), uniform(r2, nv, -scale, scale)
    return dq, dv


_RESET_STREAM = 0x5245534554 << 24  # "RESET": the engine's Philox stream of the reset noise (csrc/k_physics.hip kStreamReset)


def _philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on NumPy arrays (the device code is csrc/philox.h)."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) for x in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def reset_noise_philox(seed: int, rank: int, event: int, num_envs: int, nq: int, nv: int, scale: float):
    """The same noise from the engine's own stream (`training.rng_impl=philox`): element i (qpos words, then qvel words) of local environment n at
    event `event` is word i & 3 of philox(counter = (n, event, lo(S + (i >> 2)), hi(S)), key = seed), S = "RESET" << 24 + (rank << 16); bits become
    a float as `uniform` makes one.  Events: 0 is the reset, step t of update u is u * T + 1 + t -> float32 [N, nq], [N, nv]."""
    ne = nq + nv
    nblk = (ne + 3) // 4
    n = np.repeat(np.arange(num_envs, dtype=np.uint64), nblk)
    st = np.uint64(_RESET_STREAM + (int(rank) << 16)) + np.tile(np.arange(nblk, dtype=np.uint64), num_envs)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = np.stack(_philox4x32(n, np.full_like(n, int(event) & 0xFFFFFFFF), st & np.uint64(0xFFFFFFFF), st >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32), 1)
    bits = z.reshape(num_envs, nblk * 4)[:, :ne].astype(np.uint32)
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    lo, hi = np.float32(-scale), np.float32(scale)
    u = np.maximum(lo, f * (hi - lo) + lo).astype(np.float32)
    return u[:, :nq].copy(), u[:, nq:].copy()


_PUSH_STREAM = 0x50555348 << 24  # "PUSH": the Philox stream of the random pushes (csrc/push.h kStreamPush)


def push_wrench_philox(seed: int, rank: int, step: int, num_envs: int, force: float, interval: int, duration: int) -> np.ndarray:
    """The wrench (force xyz, torque xyz) the random pushes put on every local environment at env step `step` (csrc/push.h, bit for bit what
    `mppo_push_fill` writes and the environment kernel draws): with S = "PUSH" << 24 + (rank << 16), environment n has the phase
    word0(philox((n, 0xFFFFFFFF, lo(S), hi(S)), seed)) mod interval, is pushed iff (step + phase) mod interval < duration, and then gets
    fx, fy = uniform(word0 / word1 of philox((n, (step + phase) // interval, lo(S), hi(S)), seed), -force, force); everything else is an exact zero.
    Steps: the engine's step t of update u is u * T + t, the evaluator's is t (seed: the evaluation's, rank 0) -> float32 [N, 6]."""
    if not (force >= 0 and interval >= 1 and 1 <= duration <= interval):
        raise ValueError(f"push: force {force} / interval {interval} / duration {duration}")
    n = np.arange(num_envs, dtype=np.uint64)
    st = _PUSH_STREAM + (int(rank) << 16)
    s0, s1 = np.full_like(n, st & 0xFFFFFFFF), np.full_like(n, st >> 32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    phase = _philox4x32(n, np.full_like(n, 0xFFFFFFFF), s0, s1, k0, k1)[0] % np.uint64(interval)
    at = (np.uint64(int(step) & 0xFFFFFFFF) + phase) & np.uint64(0xFFFFFFFF)
    on = at % np.uint64(interval) < np.uint64(duration)
    z = _philox4x32(n, at // np.uint64(interval), s0, s1, k0, k1)
    bits = np.stack(z[:2], 1).astype(np.uint32)
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    lo, hi = np.float32(-force), np.float32(force)
    out = np.zeros((num_envs, 6), np.float32)
    out[:, :2] = np.where(on[:, None], np.maximum(lo, f * (hi - lo) + lo).astype(np.float32), np.float32(0.0))
    return out


_LIMIT_STREAM = 0x4C494D4954 << 24  # "LIMIT": the Philox stream of the episode time limit's stagger (csrc/limit.h kStreamLimit)


def time_limit_first_philox(seed: int, rank: int, n: int, L: int) -> np.ndarray:
    """The length at which the staggered episode time limit (`environment.episode_length` = L with `episode_length_stagger`) cuts the FIRST episode of each
    of a rank's `n` local environments (csrc/limit.h limit_first, bit for bit what `mppo_env_time_limit` tests): with S = "LIMIT" << 24 + (rank << 16),
    first_k = 1 + word0(philox((k, 0xFFFFFFFE, lo(S), hi(S)), seed)) mod L - every one in 1 .. L; every later episode is cut at L -> int64 [n]."""
    if not L >= 1:
        raise ValueError(f"time limit: episode length {L}")
    k = np.arange(n, dtype=np.uint64)
    st = _LIMIT_STREAM + (int(rank) << 16)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = _philox4x32(k, np.full_like(k, 0xFFFFFFFE), np.full_like(k, st & 0xFFFFFFFF), np.full_like(k, st >> 32), seed & 0xFFFFFFFF, seed >> 32)[0]
    return (1 + (w.astype(np.uint64) & np.uint64(0xFFFFFFFF)) % np.uint64(L)).astype(np.int64)


_DOMAIN_STREAM = 0x4452414E44 << 24  # "DRAND": the Philox stream of the domain randomisation (csrc/domrand.h kStreamDomain)


def domain_params_philox(seed: int, rank: int, num_envs: int, friction=(1.0, 1.0), actuator=(1.0, 1.0), mass=(0.0, 0.0)) -> np.ndarray:
    """The table of the domain randomisation (csrc/domrand.h, bit for bit what `mppo_domain_fill` writes): row n = (friction_scale, actuator_scale,
    added_mass, 0) with S = "DRAND" << 24 + (rank << 16), r = philox((n, 0xFFFFFFFD, lo(S), hi(S)), seed) and the three values
    uniform(r[0], *friction), uniform(r[1], *actuator), uniform(r[2], *mass); min == max gives exactly that value.  The engine draws with its configuration's
    seed and rank, the evaluator with the evaluation's seed as rank 0 -> float32 [N, 4]."""
    for name, (lo, hi) in (("friction", friction), ("actuator", actuator), ("mass", mass)):
        if not lo <= hi or (name != "mass" and lo < 0):
            raise ValueError(f"domain randomisation: {name} range {lo} .. {hi}")
    n = np.arange(num_envs, dtype=np.uint64)
    st = _DOMAIN_STREAM + (int(rank) << 16)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = _philox4x32(n, np.full_like(n, 0xFFFFFFFD), np.full_like(n, st & 0xFFFFFFFF), np.full_like(n, st >> 32), seed & 0xFFFFFFFF, seed >> 32)
    out = np.zeros((num_envs, 4), np.float32)
    for k, (lo, hi) in enumerate((friction, actuator, mass)):
        bits = z[k].astype(np.uint32)
        f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
        lo, hi = np.float32(lo), np.float32(hi)
        out[:, k] = np.maximum(lo, f * (hi - lo) + lo).astype(np.float32)
    return out


_OBS_NOISE_STREAM = 0x4F4E4F4953 << 24  # "ONOIS": the Philox stream of the sensor noise (csrc/sensor.h kStreamObsNoise)


def obs_noise_philox(seed: int, rank: int, step: int, num_envs: int, sigma) -> np.ndarray:
    """The noise the sensor-noise stage adds to the observation rows of env step `step` (csrc/sensor.h, bit for bit what `mppo_obs_noise_apply` adds): with
    S = "ONOIS" << 24 + (rank << 16), column j of local environment n gets uniform(word j & 3 of philox((n, step, lo(S) + (j >> 2), hi(S)), seed), -sigma[j],
    sigma[j]); a column whose sigma is 0 gets an exact 0 here and is NOT WRITTEN by the kernel (so `obs + noise` in float32 is the kernel's row up to the sign
    of a zero in such a column).  Steps: 0 is the row a reset writes, the engine's step t of update u is u * T + t + 1, the evaluator's step k is k + 1 (seed:
    the evaluation's, rank 0) -> float32 [N, O]."""
    sigma = np.asarray(sigma, np.float32).reshape(-1)
    if not np.all(sigma >= 0):
        raise ValueError("observation noise: a scale is negative (or not a number)")
    O = sigma.size
    nblk = (O + 3) // 4
    if nblk > 65536:
        raise ValueError(f"observation noise: {O} columns (the block index has 16 bits)")
    n = np.repeat(np.arange(num_envs, dtype=np.uint64), nblk)
    st = _OBS_NOISE_STREAM + (int(rank) << 16)
    s0 = (np.uint64(st & 0xFFFFFFFF) + np.tile(np.arange(nblk, dtype=np.uint64), num_envs)) & np.uint64(0xFFFFFFFF)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = np.stack(_philox4x32(n, np.full_like(n, int(step) & 0xFFFFFFFF), s0, np.full_like(n, st >> 32), seed & 0xFFFFFFFF, seed >> 32), 1)
    bits = z.reshape(num_envs, nblk * 4)[:, :O].astype(np.uint32)
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    lo, hi = -sigma, sigma
    u = np.maximum(lo, (f * (hi - lo)).astype(np.float32) + lo).astype(np.float32)
    return np.where(sigma > 0, u, np.float32(0.0)).astype(np.float32)


_DELAY_STREAM = 0x44454C4159 << 24  # "DELAY": the Philox stream of the actuation latency (csrc/sensor.h kStreamDelay)


def action_delays_philox(seed: int, rank: int, num_envs: int, dmin: int, dmax: int) -> np.ndarray:
    """The actuation latency, in env steps, of each of a rank's `num_envs` local environments for the whole run (csrc/sensor.h delay_draw, bit for bit what
    `mppo_action_delay_fill` writes): with S = "DELAY" << 24 + (rank << 16), d_n = dmin + word0(philox((n, 0xFFFFFFFC, lo(S), hi(S)), seed)) mod (dmax - dmin + 1).
    The engine draws with its configuration's seed and rank, the evaluator with the evaluation's seed as rank 0 -> int32 [N]."""
    if not 0 <= dmin <= dmax <= 16:
        raise ValueError(f"action delay: {dmin} .. {dmax} (0 <= min <= max <= 16)")
    n = np.arange(num_envs, dtype=np.uint64)
    st = _DELAY_STREAM + (int(rank) << 16)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = _philox4x32(n, np.full_like(n, 0xFFFFFFFC), np.full_like(n, st & 0xFFFFFFFF), np.full_like(n, st >> 32), seed & 0xFFFFFFFF, seed >> 32)[0]
    return (dmin + (w & np.uint64(0xFFFFFFFF)) % np.uint64(dmax - dmin + 1)).astype(np.int32)
