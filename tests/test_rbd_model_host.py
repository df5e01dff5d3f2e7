"""CPU tier: the host side of the batched rigid-body model (cmpc_amd/rbd.py) on tests/golden/hrp4.urdf -- the parser, the
dof order, the merging of fixed links, and the refusals."""
import re

import numpy as np
import pytest

import rbd_common as rc
import rbd_reference as ref
from cmpc_amd import rbd, workloads as wl


def test_hrp4_has_24_joints_in_urdf_order():
    m = rc.model("hrp4")
    assert len(m.joint_names) == 24 and len(m.dof_names) == 30
    names = m.dof_names
    assert names[6:12] == ('R_HIP_Y', 'R_HIP_R', 'R_HIP_P', 'R_KNEE_P', 'R_ANKLE_P', 'R_ANKLE_R')
    assert names[12:18] == ('L_HIP_Y', 'L_HIP_R', 'L_HIP_P', 'L_KNEE_P', 'L_ANKLE_P', 'L_ANKLE_R')
    assert all(n.startswith('CHEST') for n in names[18:20]) and all(n.startswith('NECK') for n in names[20:22])
    assert all(n.startswith('R_') for n in names[22:26]) and all(n.startswith('L_') for n in names[26:30])
    sel = m.joint_selection(rbd.HRP4_REDUNDANT_DOFS)
    assert np.nonzero(sel)[0].tolist() == list(range(20, 30)) and set(sel) == {0.0, 1.0}
    assert all(0 <= m.parent[i] < i for i in range(1, 25)) and m.parent[0] == -1


def test_total_mass_is_the_workloads_constant():
    assert abs(rc.model("hrp4").total_mass - wl.HRP4_MASS) < 1e-12


def test_standing_pose_reproduces_the_golden_sole_positions():
    m, q = rc.model("hrp4"), rc.standing()
    with open(rc.URDF.replace("hrp4.urdf", "pos_lfoot_pre_trj.txt")) as f:
        golden_y = float(f.readline().split()[1])
    assert golden_y == 0.10163857612916291
    f = m.frame_poses(q)
    for name, sign in (("lfoot", 1.0), ("rfoot", -1.0)):
        R, p = f[name]
        print(name, repr(p), np.abs(R - np.eye(3)).max())
        assert abs(p[1] - sign * golden_y) <= 1e-15 and abs(p[0]) <= 1e-15 and abs(p[2]) <= 1e-15
        assert np.abs(R - np.eye(3)).max() <= 1e-15
    assert abs(f['com'][2] - 0.723981584) <= 1e-8


def test_merged_tables_agree_with_the_raw_tree():
    """The reference on all 55 links of the URDF and on the 25 merged bodies: the same robot."""
    raw = rc.reference("hrp4")
    assert len(rc.raw_tree("hrp4").links) == 55
    q, v = rc.sample("hrp4")
    merged = ref.evaluate_batch(ref.tree_from_model(rc.model("hrp4")), q[:3], v[:3], rc.G)
    for k in rc.FIELDS:
        a, b = getattr(merged, k), getattr(raw, k)[:3]
        assert np.abs(a - b).max() <= rc.LEVEL * max(1.0, np.abs(b).max()), k


def _edited_urdf(tmp_path, edit):
    text = edit(open(rc.URDF).read())
    path = tmp_path / "edited.urdf"
    path.write_text(text)
    return str(path)


def test_a_tree_with_23_joints_is_refused(tmp_path):
    path = _edited_urdf(tmp_path, lambda s: s.replace('<joint name="L_ELBOW_P" type="revolute">', '<joint name="L_ELBOW_P" type="fixed">'))
    with pytest.raises(ValueError, match="exactly 24"):
        rbd.RobotModel.from_urdf(path)


def test_a_prismatic_joint_is_refused(tmp_path):
    path = _edited_urdf(tmp_path, lambda s: s.replace('<joint name="L_ELBOW_P" type="revolute">', '<joint name="L_ELBOW_P" type="prismatic">'))
    with pytest.raises(ValueError, match="prismatic"):
        rbd.RobotModel.from_urdf(path)


def _tables(**over):
    m = rc.model("hrp4")
    t = dict(parent=m.parent.copy(), joint_R=m.joint_R.copy(), joint_p=m.joint_p.copy(), axis=m.axis.copy(), mass=m.mass.copy(),
             com=m.com.copy(), inertia=m.inertia.copy(), frame_body=m.frame_body.copy(), frame_R=m.frame_R.copy(),
             frame_p=m.frame_p.copy())
    for k, (idx, val) in over.items():
        t[k][idx] = val
    return t


@pytest.mark.parametrize("over, message", [
    (dict(parent=(3, 3)), "parent"), (dict(parent=(5, 9)), "parent"), (dict(inertia=((7, 2), np.nan)), "inertia"),
    (dict(axis=(4, 0.0)), "ax"), (dict(mass=(2, -1.0)), "mass"), (dict(frame_body=(1, 25)), "frame"),
    (dict(frame_R=((2, 0, 0), 1.5)), "frame rotations"), (dict(joint_R=((6, 1, 1), 0.5)), "joint rotations")])
def test_bad_tables_are_refused_by_the_model_and_by_the_native_validation(over, message):
    t = _tables(**over)
    with pytest.raises(ValueError, match=message):
        rbd.RobotModel(**t)
    # the native validation (the one in front of the kernel's arrays) on the same tables, through the emulation's entry
    arrays = [np.ascontiguousarray(t[k]) for k in ("parent", "joint_R", "joint_p", "axis", "mass", "com", "inertia",
                                                   "frame_body", "frame_R", "frame_p")]
    q, v = rc.sample("hrp4")
    with pytest.raises(ValueError, match=message):
        rc.emulate_tables(arrays, q[:1], v[:1])
