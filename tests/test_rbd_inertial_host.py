"""CPU tier: payloads.  ``rbd.attach_payload`` merges a rigid mass into a body's inertial words by the parallel-axis rule;
here the emulated per-instance kernel on such rows is held against the independent reference on a tree that carries the
payload as ONE EXTRA LINK (no parallel-axis rule anywhere), and the whole-body QP (oracle.wbc_qp_oracle, as
tests/test_rbd_wbc_host.py uses it) has to carry the heavier robot's weight on its feet -- which it does not if the
evaluation does not read the table.  Then the helper's own contract, and ``RobotModel.body_of``."""
import functools

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import rbd_common as rc
import rbd_inertial_common as ic
import rbd_reference as ref
from cmpc_amd import rbd
from oracle import wbc_qp_oracle as wq
from wbc_tasks_common import FLAGS, literal_cost

D, MU = 0.05, 0.5
#: (kg, point of the torso body): the reference's box masses in front of the chest, a heavier one, and one off to the side
CASES = ((0.7, ic.PAYLOAD_AT), (2.0, ic.PAYLOAD_AT), (2.5, ic.PAYLOAD_AT), (5.0, ic.PAYLOAD_AT), (2.5, (0.0, 0.2, 0.1)))


@functools.lru_cache(maxsize=None)
def standing_with(mass, at):
    """The emulated per-instance kernel on the standing robot (v = 0) with that payload; read-only."""
    q = rc.standing()[None, :]
    e = ic.emulate("hrp4", q, np.zeros_like(q), ic.payload_rows([mass], at))
    for a in e:
        a.setflags(write=False)
    return e


@pytest.mark.parametrize("mass,at", CASES)
def test_merged_payload_matches_the_reference_with_one_extra_link(mass, at):
    q = rc.standing()[None, :]
    want = ref.evaluate_batch(ic.tree_with_payload(mass, at), q, np.zeros_like(q), rc.G)
    w = rc.worst(standing_with(mass, at), want)
    print(mass, at, "error / level:", w)
    assert max(w.values()) <= 1.0, w
    # (and the payload is there: the nominal robot misses the same reference)
    assert max(rc.worst(rc.emulate("hrp4", q, np.zeros_like(q)), want).values()) > 1e3


def test_merged_payload_matches_the_reference_in_motion():
    """The same with v != 0 on drawn configurations, so that the bias terms see the merged inertia too."""
    q, v = rc.sample("hrp4", 8)
    got = ic.emulate("hrp4", q[:3], v[:3], np.tile(ic.payload_rows([2.5])[0], (3, 1, 1)))
    want = ref.evaluate_batch(ic.tree_with_payload(2.5, ic.PAYLOAD_AT), q[:3], v[:3], rc.G)
    w = rc.worst(got, want)
    print("error / level:", w)
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("mass", [0.7, 2.0, 2.5])
def test_the_qp_feels_the_weight(mass):
    """Standing HRP-4 in double support with the payload on the torso: the feet carry the robot AND the box."""
    e = standing_with(mass, ic.PAYLOAD_AT)
    sel = rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS)
    zeros = np.zeros(51)
    assert np.abs(e.jdqd).max() == 0.0
    Hq, Fq = literal_cost(e.J[0], None, zeros, zeros, zeros, None, sel)
    fl, fr = FLAGS["ds"]
    r = wq.solve(Hq, Fq, e.M[0], e.h[0], np.vstack([fl * e.J[0][0:6], fr * e.J[0][6:12]]), D, MU)
    total = ic.sequential_total(ic.payload_rows([mass])[0])
    assert abs(total - (rc.model("hrp4").total_mass + mass)) < 1e-12
    fz = r["f"][5] + r["f"][11]
    print(mass, "status", r["status"], "sum fz - total g", fz - total * rc.G, "if the payload were ignored",
          fz - rc.model("hrp4").total_mass * rc.G, "max|qdd|", np.abs(r["qdd"]).max())
    assert r["status"] == 0
    assert abs(fz - total * rc.G) < 1.0
    assert np.abs(r["qdd"]).max() < 0.1


# ---- attach_payload ---------------------------------------------------------------------------------------------------------------
def test_zero_mass_returns_the_input_bits_and_a_new_array():
    tab = ic.rows("chain")
    out = rbd.attach_payload(tab, 7, 0.0, (0.1, 0.2, 0.3), inertia=np.eye(3))
    assert ic.bits_equal(out, tab) and out is not tab and out.flags.writeable
    one = rbd.attach_payload(rc.model("hrp4").inertial(), 0, 0.0, (0.0, 0.0, 0.0))
    assert one.shape == (25, 10) and ic.bits_equal(one, rc.model("hrp4").inertial())


def test_total_mass_adds_and_only_the_body_changes():
    tab = rc.model("hrp4").inertial()
    out = rbd.attach_payload(tab, 3, 1.25, (0.05, -0.02, 0.1))
    assert abs(out[:, 0].sum() - (tab[:, 0].sum() + 1.25)) < 1e-12
    assert ic.bits_equal(np.delete(out, 3, axis=0), np.delete(tab, 3, axis=0)) and not np.array_equal(out[3], tab[3])
    # the centre of mass moves towards the payload along the line between them
    d0, d1 = np.array((0.05, -0.02, 0.1)) - tab[3, 1:4], out[3, 1:4] - tab[3, 1:4]
    assert np.abs(np.cross(d0, d1)).max() < 1e-15 and abs(np.linalg.norm(d1) / np.linalg.norm(d0) - 1.25 / out[3, 0]) < 1e-12


def test_the_payloads_own_inertia_is_added_in_both_spellings():
    tab = rc.model("star").inertial()
    A = np.random.default_rng(3).normal(size=(3, 3))
    I = 0.01 * (A @ A.T + np.eye(3))
    point = rbd.attach_payload(tab, 4, 0.8, (0.1, 0.0, 0.0))
    full = rbd.attach_payload(tab, 4, 0.8, (0.1, 0.0, 0.0), inertia=I)
    six = rbd.attach_payload(tab, 4, 0.8, (0.1, 0.0, 0.0), inertia=(I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]))
    assert ic.bits_equal(full, six)
    assert np.abs(full[4, 4:] - point[4, 4:] - np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])).max() < 1e-15
    assert ic.bits_equal(full[:, :4], point[:, :4])


def test_a_sweep_is_one_call():
    tab, t = rc.model("hrp4").inertial(), ic.torso()
    masses = np.array((0.0,) + ic.PAYLOADS)
    sweep = rbd.attach_payload(tab, t, masses, ic.PAYLOAD_AT)
    assert sweep.shape == (6, 25, 10) and ic.bits_equal(sweep[0], tab)
    assert sweep.flags.c_contiguous and sweep.flags.writeable                 # (goes to the device as it is)
    for k, m in enumerate(masses):
        assert ic.bits_equal(sweep[k], rbd.attach_payload(tab, t, float(m), ic.PAYLOAD_AT)), k
    # body and at broadcast as well, over a batch of tables
    bodies, ats = np.array([1, 5, 9]), np.array([[0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1]])
    batch = rbd.attach_payload(ic.rows("star")[:3], bodies, 0.5, ats)
    for k in range(3):
        assert ic.bits_equal(batch[k], rbd.attach_payload(ic.rows("star")[k], int(bodies[k]), 0.5, ats[k])), k


def test_bad_arguments_are_refused():
    tab = rc.model("hrp4").inertial()
    for args, what in (((tab[:, :9], 0, 1.0, (0, 0, 0)), "inertial"), ((tab, 25, 1.0, (0, 0, 0)), "body"), ((tab, 1.5, 1.0, (0, 0, 0)), "body"),
                       ((tab, 0, -1.0, (0, 0, 0)), "mass"), ((tab, 0, np.nan, (0, 0, 0)), "mass"), ((tab, 0, 1.0, (0, 0)), "at"),
                       ((tab, 0, 1.0, (0, np.inf, 0)), "at")):
        with pytest.raises(ValueError, match=what):
            rbd.attach_payload(*args)
    with pytest.raises(ValueError, match="inertia"):
        rbd.attach_payload(tab, 0, 1.0, (0, 0, 0), inertia=np.zeros(5))


def test_mass_matrix_block_and_gravity_of_a_loaded_robot():
    """M[3:6,3:6] = total mass x 1 and, at rest, h[3:6] = R'(0, 0, total mass x g): the robot's own total."""
    q, _ = rc.sample("hrp4")
    tab = np.array(ic.payload_rows(np.array((0.0,) + ic.PAYLOADS + (5.0, 10.0))))
    e = ic.emulate("hrp4", q, np.zeros_like(q), tab)
    for b in range(8):
        total = ic.sequential_total(tab[b])
        assert np.array_equal(e.M[b], e.M[b].T)
        assert np.abs(e.M[b, 3:6, 3:6] - total * np.eye(3)).max() <= 1e-10
        Rb = Rotation.from_rotvec(np.array(q[b, 0:3])).as_matrix()
        assert np.abs(e.h[b, 3:6] - Rb.T @ np.array([0.0, 0.0, total * rc.G])).max() <= 1e-9 * total * rc.G
    assert np.abs(e.jdqd).max() == 0.0 and np.abs(e.vel).max() == 0.0


def test_model_inertial_and_body_of():
    m = rc.model("hrp4")
    tab = m.inertial()
    assert tab.shape == (25, 10) and tab.dtype == np.float64
    assert np.array_equal(tab[:, 0], m.mass) and np.array_equal(tab[:, 1:4], m.com) and np.array_equal(tab[:, 4:], m.inertia)
    tab[0, 0] = -1.0
    assert m.mass[0] > 0.0                                                  # (a new array)
    # the task frames' links are on the bodies the frame table names: torso on its own body, the soles merged into the ankles
    for k, name in enumerate(rbd.FRAME_ORDER):
        assert m.body_of(rbd.DEFAULT_FRAMES[name]) == int(m.frame_body[k]), name
    assert m.body_of("body") == 0 and m.body_of("torso") > 0
    assert m.body_of("l_sole") != m.body_of("r_sole") and m.body_of("l_sole") > 0
    with pytest.raises(ValueError, match="no link"):
        m.body_of("nose")
    with pytest.raises(ValueError, match="not parsed from a URDF"):
        rc.model("chain").body_of("torso")
