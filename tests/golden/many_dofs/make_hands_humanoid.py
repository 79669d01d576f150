"""Writes tests/golden/many_dofs/hands_humanoid.xml: a humanoid with a free root and two five-finger hands, 77 dofs.

Authored for this repository's tests (NOT a reference file).  It is the robot of more than 64 dofs that tests/test_many_dofs.py runs: the
dof sets of the environment kernel take a second 64-bit word here.  The arms and hands are declared BEFORE the legs, so every leg dof, the
leg limits, the leg actuators and every foot-ground contact row sit at dof indices 65 .. 76 - the path that runs every step reads the
second word.  Each finger's distal joint follows its middle joint through a joint equality (a URDF mimic joint: 10 equality rows); it
has no actuator of its own (61 actuators: the PPO engine takes at most 63).  Feet are boxes (four corner contacts each against the
ground); fingertips are spheres that meet the ground too, once the arms or the root bring them down.

    python tests/golden/many_dofs/make_hands_humanoid.py
"""
from pathlib import Path

OUT = Path(__file__).resolve().parent / "hands_humanoid.xml"

HEAD = """<!-- authored for this repository's tests (not a reference file): see tests/golden/many_dofs/make_hands_humanoid.py -->
<mujoco model="hands_humanoid">
  <compiler angle="radian" autolimits="true"/>
  <option timestep="0.002" gravity="0 0 -9.81"/>
  <default>
    <joint damping="1.0" armature="0.02"/>
    <geom contype="0" conaffinity="0" density="900" friction="0.9"/>
    <position kp="30" ctrlrange="-1 1" forcerange="-80 80"/>
    <default class="finger">
      <joint damping="0.05" armature="0.002" range="0 1.4"/>
      <position kp="2" forcerange="-3 3"/>
    </default>
    <default class="touch">
      <geom contype="1" conaffinity="0"/>
    </default>
    <default class="mimic">
      <equality solref="0.01 1"/>
    </default>
  </default>
  <worldbody>
    <geom name="floor" type="plane" size="10 10 0.1" contype="1" conaffinity="1"/>
    <body name="pelvis" pos="0 0 0.973">
      <freejoint name="root"/>
      <geom type="box" size="0.08 0.13 0.06"/>
      <body name="torso" pos="0 0 0.1">
        <joint name="waist_z" axis="0 0 1" range="-0.8 0.8"/>
        <joint name="waist_y" axis="0 1 0" range="-0.5 0.9"/>
        <joint name="waist_x" axis="1 0 0" range="-0.4 0.4"/>
        <geom type="capsule" size="0.1" fromto="0 0 0.05 0 0 0.35"/>
        <body name="head" pos="0 0 0.47">
          <joint name="neck_z" axis="0 0 1" range="-1.2 1.2"/>
          <joint name="neck_y" axis="0 1 0" range="-0.6 0.6"/>
          <geom type="sphere" size="0.09"/>
        </body>
"""

TAIL = """      </body>
{legs}    </body>
  </worldbody>
  <equality>
{equality}  </equality>
  <actuator>
{actuators}  </actuator>
</mujoco>
"""


def arm(side: str, sy: float, ind: str) -> tuple[str, list[str], list[str]]:
    """One arm with its hand under the torso: shoulder (3), elbow, wrist (3), four fingers and a thumb (4 joints each)."""
    p = side[0]
    joints_act, eqs = [], []
    x = []
    x.append(f'{ind}<body name="{p}_upper_arm" pos="0 {0.22 * sy:.2f} 0.36">')
    x.append(f'{ind}  <joint name="{p}_shoulder_y" axis="0 1 0" range="-2.0 1.2"/>')
    x.append(f'{ind}  <joint name="{p}_shoulder_x" axis="1 0 0" range="{"-0.3 2.4" if sy > 0 else "-2.4 0.3"}"/>')
    x.append(f'{ind}  <joint name="{p}_shoulder_z" axis="0 0 1" range="-1.2 1.2"/>')
    x.append(f'{ind}  <geom type="capsule" size="0.04" fromto="0 0 0 0 0 -0.28"/>')
    x.append(f'{ind}  <body name="{p}_forearm" pos="0 0 -0.28">')
    x.append(f'{ind}    <joint name="{p}_elbow" axis="0 1 0" range="-2.3 0"/>')
    x.append(f'{ind}    <geom type="capsule" size="0.035" fromto="0 0 0 0 0 -0.25"/>')
    x.append(f'{ind}    <body name="{p}_palm" pos="0 0 -0.25">')
    x.append(f'{ind}      <joint name="{p}_wrist_z" axis="0 0 1" range="-1.5 1.5"/>')
    x.append(f'{ind}      <joint name="{p}_wrist_y" axis="0 1 0" range="-1.0 1.0"/>')
    x.append(f'{ind}      <joint name="{p}_wrist_x" axis="1 0 0" range="-0.6 0.6"/>')
    x.append(f'{ind}      <geom type="box" size="0.045 0.015 0.05" pos="0 0 -0.05"/>')
    joints_act += [f"{p}_shoulder_y", f"{p}_shoulder_x", f"{p}_shoulder_z", f"{p}_elbow", f"{p}_wrist_z", f"{p}_wrist_y", f"{p}_wrist_x"]
    fingers = [("index", 0.033, -0.1, 0.045), ("middle", 0.011, -0.1, 0.05), ("ring", -0.011, -0.1, 0.045), ("little", -0.033, -0.1, 0.038),
               ("thumb", 0.05, -0.035, 0.04)]
    for fname, fx, fz, l1 in fingers:
        f = f"{p}_{fname}"
        thumb = fname == "thumb"
        l2, l3 = 0.7 * l1, 0.5 * l1
        i2 = ind + "      "
        x.append(f'{i2}<body name="{f}_prox" pos="{fx} {-0.02 * sy if thumb else 0.0:.3f} {fz}" childclass="finger">')
        x.append(f'{i2}  <joint name="{f}_abd" axis="{"0 0 1" if thumb else "0 1 0"}" range="-0.35 0.35"/>')
        x.append(f'{i2}  <joint name="{f}_mcp" axis="1 0 0"/>')
        x.append(f'{i2}  <geom type="capsule" size="0.009" fromto="0 0 0 0 0 {-l1:.3f}"/>')
        x.append(f'{i2}  <body name="{f}_mid" pos="0 0 {-l1:.3f}">')
        x.append(f'{i2}    <joint name="{f}_pip" axis="1 0 0"/>')
        x.append(f'{i2}    <geom type="capsule" size="0.008" fromto="0 0 0 0 0 {-l2:.3f}"/>')
        x.append(f'{i2}    <body name="{f}_dist" pos="0 0 {-l2:.3f}">')
        x.append(f'{i2}      <joint name="{f}_dip" axis="1 0 0"/>')
        x.append(f'{i2}      <geom type="capsule" size="0.007" fromto="0 0 0 0 0 {-l3:.3f}"/>')
        x.append(f'{i2}      <geom type="sphere" size="0.009" pos="0 0 {-l3:.3f}" class="touch"/>')
        x.append(f'{i2}    </body>')
        x.append(f'{i2}  </body>')
        x.append(f'{i2}</body>')
        joints_act += [f"{f}_abd", f"{f}_mcp", f"{f}_pip"]
        eqs.append(f'    <joint name="{f}_mimic" class="mimic" joint1="{f}_dip" joint2="{f}_pip" polycoef="0 0.8 0 0 0"/>')
    x.append(f'{ind}    </body>')
    x.append(f'{ind}  </body>')
    x.append(f'{ind}</body>')
    return "\n".join(x) + "\n", joints_act, eqs


def leg(side: str, sy: float, ind: str) -> tuple[str, list[str]]:
    p = side[0]
    x = [f'{ind}<body name="{p}_thigh" pos="0 {0.1 * sy:.2f} -0.05">',
         f'{ind}  <joint name="{p}_hip_z" axis="0 0 1" range="-0.7 0.7"/>',
         f'{ind}  <joint name="{p}_hip_x" axis="1 0 0" range="-0.5 0.5"/>',
         f'{ind}  <joint name="{p}_hip_y" axis="0 1 0" range="-1.6 0.6"/>',
         f'{ind}  <geom type="capsule" size="0.055" fromto="0 0 0 0 0 -0.42"/>',
         f'{ind}  <body name="{p}_shin" pos="0 0 -0.42">',
         f'{ind}    <joint name="{p}_knee" axis="0 1 0" range="0 2.4"/>',
         f'{ind}    <geom type="capsule" size="0.045" fromto="0 0 0 0 0 -0.42"/>',
         f'{ind}    <body name="{p}_foot" pos="0 0 -0.42">',
         f'{ind}      <joint name="{p}_ankle_y" axis="0 1 0" range="-0.8 0.8"/>',
         f'{ind}      <joint name="{p}_ankle_x" axis="1 0 0" range="-0.4 0.4"/>',
         f'{ind}      <geom type="box" size="0.1 0.045 0.025" pos="0.03 0 -0.06" class="touch"/>',
         f'{ind}    </body>',
         f'{ind}  </body>',
         f'{ind}</body>']
    return "\n".join(x) + "\n", [f"{p}_hip_z", f"{p}_hip_x", f"{p}_hip_y", f"{p}_knee", f"{p}_ankle_y", f"{p}_ankle_x"]


def text() -> str:
    body, acts, eqs = HEAD, ["waist_z", "waist_y", "waist_x", "neck_z", "neck_y"], []
    for side, sy in (("left", 1.0), ("right", -1.0)):
        a, j, e = arm(side, sy, "        ")
        body += a
        acts += j
        eqs += e
    legs = ""
    for side, sy in (("left", 1.0), ("right", -1.0)):
        lg, j = leg(side, sy, "      ")
        legs += lg
        acts += j
    fingers = {"abd", "mcp", "pip"}
    lines = [f'    <position joint="{j}"{" class=" + chr(34) + "finger" + chr(34) if j.rsplit("_", 1)[-1] in fingers else ""}/>' for j in acts]
    return body + TAIL.format(legs=legs, equality="\n".join(eqs) + "\n", actuators="\n".join(lines) + "\n")


if __name__ == "__main__":
    OUT.write_text(text())
    print(f"wrote {OUT}")
