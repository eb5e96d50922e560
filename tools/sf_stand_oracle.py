import os, sys; sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from tests import physics_harness as ph
built = ph.build(ph.PhysicsCase("tron1_sf", "TRON1SFCfg", n=1), 0)
model = built.model
arm = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
for k in range(8): built.desc.armature[k] = arm
st = ph.floating_state(built, 1, 0.84)
st.arr["added_base_mass"][:] = 0
orc = ph.OracleStepper(built, "f64")
orc.load(st); st = orc.st
act = np.zeros((1, 8), np.float32)
L = model.n_links
for k in range(300):
    orc.step(act)
    if k % 25 == 0 or k > 296:
        f = st.arr["link_contact_forces"][0].reshape(L, 3)
        print(k, "z", round(float(st.arr["base_pos"][0,2]),4), "feet z", np.round(st.arr["feet_pos"][0].reshape(2,3)[:,2],4), "Fz", np.round(f[[0,3,4,7,8],2],1), "q", np.round(st.arr["dof_pos"][0][:4],3), "qd", np.round(st.arr["dof_vel"][0][:4],2), "pg", np.round(st.arr["projected_gravity"][0],2))
