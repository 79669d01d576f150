"""Builds minppo_amd/libminppo_hip.so: every HIP source in csrc/ compiled for gfx950 with hipcc.

    python -m minppo_amd.build [--force]

hipcc cross-compiles without a GPU.  Objects go to minppo_amd/csrc/_build/ (git-ignored); the
shared library stays in-tree so that it travels to the GPU box with the repository snapshot.
"""

from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parent
CSRC = HERE / "csrc"
BUILD = CSRC / "_build"
LIB = HERE / "libminppo_hip.so"
ARCH = "gfx950"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-I" + str(CSRC), "-I" + str(HERE.parent / "include"),
         "-Wno-unused-result"]


# Per-file flags.  k_physics.hip is compiled WITHOUT floating-point contraction: measured on MI355X (tools/phys_envelope.py, 64
# walking states), fused multiply-adds everywhere move the constraint solver's result 4x further from the float64 oracle
# (median |dqacc| 3.5e-3 of scale against 9e-4; the solver is an unconverged CG that amplifies where a product was rounded)
# while saving only 4 % of the kernel's time; hot inner products use explicit fmaf where that does not cost parity.
FILE_FLAGS = {"k_physics.hip": ["-ffp-contract=off"]}
FILE_FLAGS["env_model.hip"] = FILE_FLAGS["k_physics.hip"]  # (the kernel's model handle: one list, so that the two agree on MPPO_REGCHOL_MAX_NV below)
# (k_obsnorm.hip: the running statistics' float64 merge, whose roundings the tests restate operation by operation)
FILE_FLAGS["k_obsnorm.hip"] = ["-ffp-contract=off"]
# (k_rewnorm.hip: the discounted return `ret * gamma + reward` is specified as a float32 multiply and a float32 add - two roundings, which the tests restate
# operation by operation and the engine's carry repeats from update to update; contracted to one fused multiply-add it rounds once and differs in the last bit)
FILE_FLAGS["k_rewnorm.hip"] = ["-ffp-contract=off"]
# (k_push.hip: the pushes' draw `f * (hi - lo) + lo` is a float32 multiply and a float32 add, as the host restatement and the environment kernel - compiled without
# contraction, above - compute it; fused into one multiply-add the fill kernel's last bit would differ from both)
FILE_FLAGS["k_push.hip"] = ["-ffp-contract=off"]
# (k_domrand.hip: the domain randomisation's draw, the same multiply and add - held bit-equal to its host restatement)
FILE_FLAGS["k_domrand.hip"] = ["-ffp-contract=off"]
# (k_sensor.hip: the sensor noise's draw, the same multiply and add, and the one float32 add onto the observation - held bit-equal to its host restatement)
FILE_FLAGS["k_sensor.hip"] = ["-ffp-contract=off"]
# MPPO_REGCHOL_MAX_NV=32: specialised kernels beyond 32 dofs keep their Cholesky factors in LDS instead of registers (the default, 48, is three
# matrix rows per lane: fastest, at 400 - 500 registers; the library checks every instantiation MPPO_SPECIALIZE adds against the run-time-sized
# kernel on the device and falls back if they differ)
if os.environ.get("MPPO_REGCHOL_MAX_NV"):
    FILE_FLAGS["k_physics.hip"].append("-DMPPO_REGCHOL_MAX_NV=" + str(int(os.environ["MPPO_REGCHOL_MAX_NV"])))


# Models the environment kernel is additionally compiled for with fixed dimensions (csrc/spec_dims.inc; k_physics.hip explains
# why that is faster).  The BASELINE robots by default; MPPO_SPECIALIZE="robot.xml,other_builtin" adds models for this build.
# (synth_pile: every collider kind in one robot - hull pairs, a cylinder, plane_convex - so that the specialised form of those code paths is built
# and held bit-equal to the run-time-sized one by tests/test_kernels_physics.py)
# (the export-style biped - tests/golden/export_biped, 33 dofs / 19 contact slots - since round 6: the only default instantiation beyond 32 dofs, i.e. the
# one that builds the three-rows-per-lane register Cholesky and a specialised kernel whose matrices live in global memory, and holds them bit-equal too)
# (the contact-parameter humanoid - tests/golden/contact_params_humanoid.xml: the per-row contact / limit parameter path of blob version 8, specialised)
# (the four-bar biped - tests/golden/equality/fourbar_biped.xml: the equality rows of blob version 9, specialised)
# (the ball-joint humanoid - tests/golden/ball_joints/ball_humanoid.xml: ball joints - kinematics, limit rows of three entries, springs, motors - specialised)
SPECIALIZED_MODELS = ["synth_stompy_pro", "synth_stompy_full", "synth_pile", str(HERE.parent / "tests" / "golden" / "export_biped" / "robot.xml"),
                      str(HERE.parent / "tests" / "golden" / "contact_params_humanoid.xml"), str(HERE.parent / "tests" / "golden" / "equality" / "fourbar_biped.xml"),
                      str(HERE.parent / "tests" / "golden" / "ball_joints" / "ball_humanoid.xml")]
SPEC_INC = CSRC / "spec_dims.inc"
# (the members of csrc/model_view.h BlobDims = the template parameters of k_physics.hip StaticModel, in their order)
_SPEC_KEYS = ("nq", "nv", "nu", "nbody", "njnt", "ncon", "nlimit", "npair", "nlevel", "nroot", "ncvx", "ncvxvert", "hull", "ncyl", "neq", "nball", "cparam")


def spec_dims_of(t) -> tuple:
    """A compiled model's StaticModel dims (tables: CompiledModel.t; `neq` / `nball` are absent from a model without equality constraints / ball joints)."""
    return tuple((1 if int(t["nhull"]) > 0 else 0) if k == "hull" else int(t.get(k, 0)) for k in _SPEC_KEYS)


def spec_dims_text(models: list[str], extra: list[str] = ()) -> str:
    from minppo_amd.model import load_model

    lines = [f"// Models the environment kernel is compiled for ({', '.join(_SPEC_KEYS)}): GENERATED by",
             "// minppo_amd/build.py from SPECIALIZED_MODELS (+ $MPPO_SPECIALIZE); every other model runs the run-time-sized kernel."]
    seen = set()
    for name in list(models) + list(extra):
        if name in models and name.endswith(".xml") and not Path(name).exists():
            continue  # (a default fixture robot that this source tree does not carry)
        t = load_model(name).t
        dims = spec_dims_of(t)
        if dims in seen:
            continue
        seen.add(dims)
        # (an instantiation added for this build is checked against the run-time-sized kernel on the device when a model first uses it:
        # k_physics.hip spec_self_check; the default ones are held bit-equal by the test suite)
        lines.append(f"{'MPPO_SPEC_EXTRA' if name in extra else 'MPPO_SPEC'}({', '.join(map(str, dims))})  // {Path(name).name}")
    return "\n".join(lines) + "\n"


def write_spec_dims() -> None:
    extra = [m for m in os.environ.get("MPPO_SPECIALIZE", "").split(",") if m]
    text = spec_dims_text(SPECIALIZED_MODELS, extra)
    if not SPEC_INC.exists() or SPEC_INC.read_text() != text:
        SPEC_INC.write_text(text)


def sources() -> list[Path]:
    names = (CSRC / "SOURCES.txt").read_text().split() + (CSRC / "SOURCES_DEVICE_ONLY.txt").read_text().split()
    return [CSRC / n for n in names]


def _newer(target: Path, deps: list[Path]) -> bool:
    if not target.exists():
        return False
    t = target.stat().st_mtime
    return all(d.stat().st_mtime <= t for d in deps)


def build(force: bool = False, verbose: bool = True) -> Path:
    BUILD.mkdir(exist_ok=True)
    write_spec_dims()
    headers = sorted(CSRC.glob("*.h")) + [SPEC_INC] + [HERE.parent / "include" / "minppo_hip.h", Path(__file__)]
    srcs = sources()
    objs = [BUILD / (s.stem + ".o") for s in srcs]

    def compile_one(pair):
        src, obj = pair
        if not force and _newer(obj, [src] + headers):
            return None
        cmd = [HIPCC, *FLAGS, *FILE_FLAGS.get(src.name, []), "-c", str(src), "-o", str(obj)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src.name}:\n{r.stderr[-4000:]}")
        return src.name

    with ThreadPoolExecutor(max_workers=min(6, len(srcs))) as ex:
        done = [d for d in ex.map(compile_one, zip(srcs, objs)) if d]
    if done or force or not _newer(LIB, objs):
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", str(LIB), *map(str, objs), "-L/opt/rocm/lib", "-lrccl",
               "-Wl,-rpath,/opt/rocm/lib"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    if verbose:
        print(f"[minppo_amd.build] compiled {done or 'nothing (up to date)'} -> {LIB}")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
