"""Diagnostic: tron1_sf physics, component-per-lane vs leg-per-lane kernel on the same states (airborne, then with contacts)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dataclasses
import numpy as np
from tests import physics_harness as ph
OUT = ph.SIM_OUT[:10]          # up to feet_vel
case = ph.PhysicsCase("tron1_sf", "TRON1SFCfg", n=256)
builts = [ph.build(case, lay) for lay in ph.LAYOUTS]
engs = [ph.EngineStepper(b, case.n) for b in builts]
for name, zoff in (("airborne", 2.0), ("contacts", 0.0)):
    st, actions = ph.initial_state(dataclasses.replace(case, z_offset=zoff), builts[0])
    st.arr["joint_armature"] = np.full((256, 1), 0.12, np.float32)
    st.arr["joint_friction"] = np.full((256, 1), 0.005, np.float32)
    st.arr["joint_damping"] = np.full((256, 1), 1.4, np.float32)
    res = []
    for e in engs:
        e.load(st)
        e.step(actions)
        res.append(e.arrays(OUT))
    print("==", name)
    for k in OUT:
        d = np.abs(res[0][k] - res[1][k])
        print(f"  {k:22s} max diff {d.max():.3e}  worst col {np.unravel_index(d.argmax(), d.shape)}  frac>1e-4 {(d > 1e-4).mean():.3f}")
