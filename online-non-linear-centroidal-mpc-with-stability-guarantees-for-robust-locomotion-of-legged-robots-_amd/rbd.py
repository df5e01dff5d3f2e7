"""Batched rigid-body model (include/cmpc_rbd.h, csrc/rbd_kernel.hpp): what the reference takes from DART every tick --
the task Jacobians, their bias accelerations, the mass matrix and the Coriolis + gravity vector of
code/inverse_dynamics.py:46-65, :112, :116, and the measured ``current`` of code/simulation.py:303-388 -- for B robots in
one HIP launch, in the layouts ``BatchedInverseDynamicsQP.solve_tasks`` and ``BatchedCentroidalMPC.track`` consume.

``RobotModel`` is the host side (numpy and the standard library): a kinematic tree parsed from a URDF, fixed joints merged,
validated so that no table can index outside the kernel's arrays.  ``BatchedRobot`` is the device side; there is no CPU
fallback.  ``Gait``, ``BatchedRobot.task_references``, ``integrate`` and ``walking_model`` close the loop around it
(include/cmpc_walk.h, csrc/rbd_walk_kernel.hpp): the task references of a walking robot from its own adapted plan, and the
step from the QP's acceleration to the next tick's (q, v).  ``BatchedRobot.measure`` (``cmpc_walk_measure``,
csrc/walk_measure_kernel.hpp) feeds the robot's own centroid and foot angles back into the state its MPC starts from.
``Plant`` and ``BatchedRobot.simulate`` (``cmpc_walk_plant_step``, csrc/walk_plant_kernel.hpp) are the contact plant: the QP's
torques, a wrench on the base and a flat frictional floor under the sole vertices move the robot instead of the QP's
acceleration.  ``BatchedRobot(inertial=...)`` (``cmpc_rbd_eval_inertial``, csrc/rbd_inertial.hip) gives every robot of the batch
its own link masses, centres of mass and inertias -- ``RobotModel.inertial`` is the model's row and ``attach_payload`` welds a
load to a body --, and everything above sees that robot, since it all goes through ``evaluate``.

Coordinates (this build's own: parity with DART's is not pinned by any test): q[0:3] is the rotation
vector of the base, R_b = Exp(q[0:3]) (world <- base), q[3:6] the base origin in the world, q[6+k] the joint angles in URDF
file order; v[0:3] and v[3:6] are the base angular and base-origin linear velocity in the BASE frame (the body twist),
v[6+k] the joint rates.  M, h are those of M vdot + h = S' tau + Jc' f with vdot the plain time derivative of v.
"""
import collections
import ctypes
import xml.etree.ElementTree as ET

import numpy as np

BODIES, DOFS, BASE, FRAMES, ROWS = 25, 30, 6, 4, 21
FRAME_ORDER = ('lfoot', 'rfoot', 'torso', 'base')
DEFAULT_FRAMES = {'lfoot': 'l_sole', 'rfoot': 'r_sole', 'torso': 'torso', 'base': 'body'}
BASE_DOF_NAMES = ('base_rot_x', 'base_rot_y', 'base_rot_z', 'base_pos_x', 'base_pos_y', 'base_pos_z')
#: code/simulation.py:88-91
HRP4_REDUNDANT_DOFS = ("NECK_Y", "NECK_P", "R_SHOULDER_P", "R_SHOULDER_R", "R_SHOULDER_Y", "R_ELBOW_P",
                       "L_SHOULDER_P", "L_SHOULDER_R", "L_SHOULDER_Y", "L_ELBOW_P")
#: code/simulation.py:63-67, degrees
HRP4_INITIAL_DEG = {'CHEST_P': 0., 'CHEST_Y': 0., 'NECK_P': 0., 'NECK_Y': 0.,
                    'R_HIP_Y': 0., 'R_HIP_R': -3., 'R_HIP_P': -25., 'R_KNEE_P': 50., 'R_ANKLE_P': -25., 'R_ANKLE_R': 3.,
                    'L_HIP_Y': 0., 'L_HIP_R': 3., 'L_HIP_P': -25., 'L_KNEE_P': 50., 'L_ANKLE_P': -25., 'L_ANKLE_R': -3.,
                    'R_SHOULDER_P': 4., 'R_SHOULDER_R': -8., 'R_SHOULDER_Y': 0., 'R_ELBOW_P': -25.,
                    'L_SHOULDER_P': 4., 'L_SHOULDER_R': 8., 'L_SHOULDER_Y': 0., 'L_ELBOW_P': -25.}

Evaluation = collections.namedtuple("Evaluation", "J jdqd M h pose vel centroid")
#: the outputs of ``cmpc_walk_task_refs``: rows of ``solve_tasks`` (21 task rows + 30 dofs), and the desired feet
NACC, FEET_WORDS = ROWS + DOFS, 36
References = collections.namedtuple("References", "ff pos_err vel_err feet_des")
REFERENCE_FIELDS = References._fields
#: the optional outputs of ``cmpc_walk_measure``: the measured x0 (B,20) and measured minus predicted (B,9)
Measurement = collections.namedtuple("Measurement", "x_meas innovation")
#: what ``cmpc_walk_plant_step`` returns: the next (q, v) (B,30), the contact impulses (B,24), status (B,) int32 (0 stepped,
#: 1 held, 2 refused) and the normal velocity in m/s by which the step still violates non-penetration (B,)
PlantStep = collections.namedtuple("PlantStep", "q v impulse status residual")
PLANT_OUTPUTS = ("impulse", "status", "residual")
IMPULSE_WORDS = 24


class Plant:
    """The parameters of the contact plant (``cmpc_walk_plant_params`` of include/cmpc_walk.h): the time step ``dt``, the
    number of Gauss-Seidel ``sweeps`` over the eight sole vertices, the share ``erp`` of a penetration that a tick removes,
    the diagonal term ``cfm`` of the contact matrix and the height ``ground_z`` of the floor.  The defaults are starting
    values, not validated ones: ``PlantStep.residual`` says whether the sweeps were enough.  Needs no device."""

    def __init__(self, dt, sweeps=50, erp=0.2, cfm=0.0, ground_z=0.0):
        if isinstance(sweeps, bool) or int(sweeps) != sweeps or sweeps < 0:
            raise ValueError("sweeps must be an integer >= 0")
        dt, erp, cfm, ground_z = float(dt), float(erp), float(cfm), float(ground_z)
        if not (np.isfinite(dt) and dt > 0.):
            raise ValueError("dt must be finite and > 0")
        if not 0. <= erp <= 1.:
            raise ValueError("erp must be in [0, 1]")
        if not (np.isfinite(cfm) and cfm >= 0.):
            raise ValueError("cfm must be finite and >= 0")
        if not np.isfinite(ground_z):
            raise ValueError("ground_z must be finite")
        self.dt, self.sweeps, self.erp, self.cfm, self.ground_z = dt, int(sweeps), erp, cfm, ground_z

    def params(self):
        """The ``capi.PlantParams`` of a launch."""
        from . import capi
        return capi.PlantParams(ctypes.sizeof(capi.PlantParams), self.sweeps, self.dt, self.ground_z, self.erp, self.cfm)

    def __repr__(self):
        return f"Plant(dt={self.dt}, sweeps={self.sweeps}, erp={self.erp}, cfm={self.cfm}, ground_z={self.ground_z})"


def rpy_matrix(rpy):
    """URDF's fixed-axis roll, pitch, yaw: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = (float(a) for a in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def axis_rotation(a, q):
    """Rotation by q about the unit axis a."""
    K = np.array([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]])
    return np.eye(3) + np.sin(q) * K + (1. - np.cos(q)) * (K @ K)


def exp_so3(w):
    w = np.asarray(w, dtype=np.float64)
    t = np.linalg.norm(w)
    return np.eye(3) if t == 0. else axis_rotation(w / t, t)


def _vec(text, default):
    return np.array([float(x) for x in (text.split() if text else default.split())])


def _origin(el):
    o = None if el is None else el.find('origin')
    xyz = _vec(None if o is None else o.get('xyz'), '0 0 0')
    rpy = _vec(None if o is None else o.get('rpy'), '0 0 0')
    if xyz.shape != (3,) or rpy.shape != (3,):
        raise ValueError("an <origin> needs three numbers in xyz and in rpy")
    return rpy_matrix(rpy), xyz


def _orthonormal(R):
    """R'R = I to 1e-9 for every matrix of the stack (the native validation's rule)."""
    return bool(np.all(np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)) < 1e-9))


def _sym6(I):
    return np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])


class RobotModel:
    """The validated tables of ``cmpc_rbd_model_create``: body 0 is the floating base, body i (1..24) hangs on
    ``parent[i] < i`` by a revolute joint and is moved by dof 5 + i.  ``joint_names``: the 24 joints in dof order."""

    def __init__(self, parent, joint_R, joint_p, axis, mass, com, inertia, frame_body, frame_R, frame_p, joint_names=None):
        f64 = np.float64
        self.parent = np.ascontiguousarray(parent, dtype=np.int32)
        self.joint_R = np.ascontiguousarray(joint_R, dtype=f64)
        self.joint_p = np.ascontiguousarray(joint_p, dtype=f64)
        self.axis = np.array(axis, dtype=f64, order='C')
        self.mass = np.ascontiguousarray(mass, dtype=f64)
        self.com = np.ascontiguousarray(com, dtype=f64)
        self.inertia = np.ascontiguousarray(inertia, dtype=f64)
        self.frame_body = np.ascontiguousarray(frame_body, dtype=np.int32)
        self.frame_R = np.ascontiguousarray(frame_R, dtype=f64)
        self.frame_p = np.ascontiguousarray(frame_p, dtype=f64)
        for name, a, shape in (("parent", self.parent, (BODIES,)), ("joint_R", self.joint_R, (BODIES, 3, 3)),
                               ("joint_p", self.joint_p, (BODIES, 3)), ("axis", self.axis, (BODIES, 3)),
                               ("mass", self.mass, (BODIES,)), ("com", self.com, (BODIES, 3)),
                               ("inertia", self.inertia, (BODIES, 6)), ("frame_body", self.frame_body, (FRAMES,)),
                               ("frame_R", self.frame_R, (FRAMES, 3, 3)), ("frame_p", self.frame_p, (FRAMES, 3))):
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape}: this build serves trees with exactly {BODIES - 1} "
                                 f"one-dof joints ({DOFS} dofs with the floating base), got {a.shape}")
        if self.parent[0] != -1 or any(not (0 <= self.parent[i] < i) for i in range(1, BODIES)):
            raise ValueError("parents must be ordered: parent[0] = -1 and 0 <= parent[i] < i")
        n = np.linalg.norm(self.axis[1:], axis=1)
        if not (np.all(np.isfinite(self.axis[1:])) and np.all(n > 1e-12)):
            raise ValueError("joint axes must be finite and non-zero")
        self.axis[1:] /= n[:, None]
        self.axis[0] = (0., 0., 1.)
        if not (np.all(np.isfinite(self.joint_R)) and np.all(np.isfinite(self.joint_p))):
            raise ValueError("joint placements must be finite")
        if not _orthonormal(self.joint_R[1:]):
            raise ValueError("joint rotations must be orthonormal")
        if not (np.all(np.isfinite(self.mass)) and np.all(self.mass >= 0.) and self.mass.sum() > 0.):
            raise ValueError("masses must be finite and >= 0, with a total > 0")
        if not np.all(np.isfinite(self.inertia)):
            raise ValueError("inertias must be finite")
        if not np.all(np.isfinite(self.com)):
            raise ValueError("centres of mass must be finite")
        if not (np.all((0 <= self.frame_body) & (self.frame_body < BODIES)) and np.all(np.isfinite(self.frame_R))
                and np.all(np.isfinite(self.frame_p))):
            raise ValueError("task frames must sit on a body of the tree, with finite placements")
        if not _orthonormal(self.frame_R):
            raise ValueError("task frame rotations must be orthonormal")
        self.joint_names = tuple(joint_names) if joint_names is not None else tuple(f"joint_{i}" for i in range(BODIES - 1))
        if len(self.joint_names) != BODIES - 1:
            raise ValueError(f"{BODIES - 1} joint names expected")
        self.dof_names = BASE_DOF_NAMES + self.joint_names
        self.total_mass = float(self.mass.sum())

    # ---- parsing ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_urdf(cls, path, frames=None):
        """Parse a URDF: ``revolute`` / ``continuous`` joints give one dof each, in file order; ``fixed`` joints are merged
        into the parent body (mass, centre of mass and inertia by the parallel-axis rule, ``<inertial><origin rpy>``
        honoured; a task frame on a merged link becomes a fixed offset on the body that absorbed it); any other joint type
        is refused.  ``frames``: link names of the task frames lfoot, rfoot, torso, base."""
        frames = dict(DEFAULT_FRAMES, **(frames or {}))
        root = ET.parse(path).getroot()
        links = {}
        for el in root.findall('link'):
            ine = el.find('inertial')
            m, c, I = 0., np.zeros(3), np.zeros((3, 3))
            if ine is not None:
                R, c = _origin(ine)
                mel, iel = ine.find('mass'), ine.find('inertia')
                m = float(mel.get('value')) if mel is not None else 0.
                if iel is not None:
                    g = lambda k: float(iel.get(k, '0'))
                    I = np.array([[g('ixx'), g('ixy'), g('ixz')], [g('ixy'), g('iyy'), g('iyz')], [g('ixz'), g('iyz'), g('izz')]])
                    I = R @ I @ R.T
            links[el.get('name')] = (m, c, I)
        joints = []
        for el in root.findall('joint'):
            kind = el.get('type')
            if kind not in ('revolute', 'continuous', 'fixed'):
                raise ValueError(f"joint {el.get('name')!r}: type {kind!r} is not supported (revolute, continuous, fixed)")
            R, p = _origin(el)
            ax = el.find('axis')
            joints.append(dict(name=el.get('name'), kind=kind, R=R, p=p, parent=el.find('parent').get('link'),
                               child=el.find('child').get('link'), axis=_vec(None if ax is None else ax.get('xyz'), '1 0 0')))
        children = {j['child'] for j in joints}
        roots = [n for n in links if n not in children]
        if len(roots) != 1:
            raise ValueError(f"the URDF must have exactly one root link, found {roots}")
        moving = [j for j in joints if j['kind'] != 'fixed']
        if len(moving) != BODIES - 1:
            raise ValueError(f"this build serves trees with exactly {BODIES - 1} one-dof joints ({DOFS} dofs with the "
                             f"floating base): the URDF has {len(moving)}")
        # link -> (body, R, p): the link's frame in the body that carries it
        place = {roots[0]: (0, np.eye(3), np.zeros(3))}
        parent = np.full(BODIES, -1, dtype=np.int32)
        joint_R, joint_p = np.tile(np.eye(3), (BODIES, 1, 1)), np.zeros((BODIES, 3))
        axis = np.tile(np.array([0., 0., 1.]), (BODIES, 1))
        index = {j['name']: 1 + k for k, j in enumerate(moving)}
        pending = list(joints)
        while pending:
            ready = [j for j in pending if j['parent'] in place]
            if not ready:
                raise ValueError("the URDF's joints do not form a tree on its root link")
            for j in ready:
                if j['child'] in place:
                    raise ValueError(f"link {j['child']!r} has two parents")
                b, Rb, pb = place[j['parent']]
                R, p = Rb @ j['R'], pb + Rb @ j['p']
                if j['kind'] == 'fixed':
                    place[j['child']] = (b, R, p)
                else:
                    i = index[j['name']]
                    parent[i], joint_R[i], joint_p[i], axis[i] = b, R, p, j['axis']
                    place[j['child']] = (i, np.eye(3), np.zeros(3))
            pending = [j for j in pending if j not in ready]
        mass, com, inertia = np.zeros(BODIES), np.zeros((BODIES, 3)), np.zeros((BODIES, 6))
        for b in range(BODIES):
            parts = [(links[n][0], p + R @ links[n][1], R @ links[n][2] @ R.T) for n, (bb, R, p) in place.items() if bb == b]
            m = sum(x[0] for x in parts)
            c = sum(x[0] * x[1] for x in parts) / m if m > 0. else np.zeros(3)
            I = np.zeros((3, 3))
            for mk, ck, Ik in parts:                                          # parallel axes, to the body's centre of mass
                d = ck - c
                I = I + Ik + mk * (d @ d * np.eye(3) - np.outer(d, d))
            mass[b], com[b], inertia[b] = m, c, _sym6(I)
        fb, fR, fp = np.zeros(FRAMES, dtype=np.int32), np.zeros((FRAMES, 3, 3)), np.zeros((FRAMES, 3))
        for k, name in enumerate(FRAME_ORDER):
            if frames[name] not in place:
                raise ValueError(f"task frame {name!r}: the URDF has no link {frames[name]!r}")
            fb[k], fR[k], fp[k] = place[frames[name]]
        model = cls(parent, joint_R, joint_p, axis, mass, com, inertia, fb, fR, fp, joint_names=[j['name'] for j in moving])
        model.link_body = {n: int(b) for n, (b, _, _) in place.items()}
        return model

    # ---- host helpers ----------------------------------------------------------------------------------------------------
    def tables(self):
        """The arrays of ``cmpc_rbd_model_create``, in its argument order."""
        return (self.parent, self.joint_R, self.joint_p, self.axis, self.mass, self.com, self.inertia, self.frame_body,
                self.frame_R, self.frame_p)

    def inertial(self):
        """The model's inertial table (25, 10): per body mass, centre of mass xyz, inertia xx xy xz yy yz zz -- one robot's
        row of ``BatchedRobot(inertial=...)`` (a new array)."""
        return np.concatenate([self.mass[:, None], self.com, self.inertia], axis=1)

    def body_of(self, link_name):
        """The body (0..24) that carries the URDF link ``link_name``: the link's own if a moving joint leads to it, otherwise
        the one it was merged into.  Only a model that ``from_urdf`` parsed knows its links."""
        links = getattr(self, "link_body", None)
        if links is None:
            raise ValueError("this model was not parsed from a URDF: it has no link names")
        if link_name not in links:
            raise ValueError(f"the URDF has no link {link_name!r}")
        return links[link_name]

    def joint_selection(self, names):
        """The diagonal (30,) of ``joint_selection`` (code/inverse_dynamics.py:24-28): 1 at the dofs named."""
        sel = np.zeros(DOFS)
        for n in names:
            sel[self.dof_names.index(n)] = 1.
        return sel

    def configuration(self, angles, degrees=False):
        """q (30,) with the base at the origin and the joints named in ``angles`` set (the others 0)."""
        q = np.zeros(DOFS)
        for n, a in angles.items():
            q[self.dof_names.index(n)] = np.deg2rad(a) if degrees else a
        return q

    def body_poses(self, q):
        """World rotations (25,3,3) and origins (25,3) of the bodies at q (30,): plain forward kinematics on the host."""
        q = np.asarray(q, dtype=np.float64)
        R, p = np.zeros((BODIES, 3, 3)), np.zeros((BODIES, 3))
        R[0], p[0] = exp_so3(q[0:3]), q[3:6]
        for i in range(1, BODIES):
            k = self.parent[i]
            R[i] = R[k] @ self.joint_R[i] @ axis_rotation(self.axis[i], q[5 + i])
            p[i] = p[k] + R[k] @ self.joint_p[i]
        return R, p

    def frame_poses(self, q):
        """name -> (R (3,3), p (3,)) of the task frames at q, and 'com' -> p."""
        R, p = self.body_poses(q)
        out = {n: (R[b] @ self.frame_R[k], p[b] + R[b] @ self.frame_p[k]) for k, (n, b) in enumerate(zip(FRAME_ORDER, self.frame_body))}
        out['com'] = sum(self.mass[i] * (p[i] + R[i] @ self.com[i]) for i in range(BODIES)) / self.total_mass
        return out

    def place_on_ground(self, q):
        """q with the base origin moved so that the midpoint of the soles is the world origin (code/simulation.py:73-77)."""
        q = np.array(q, dtype=np.float64)
        f = self.frame_poses(q)
        q[3:6] -= (f['lfoot'][1] + f['rfoot'][1]) / 2.
        return q


INERTIAL_WORDS = 10


def _parallel_axes(m, d):
    """m (|d|^2 1 - d d') as xx xy xz yy yz zz: m (...,), d (...,3) -> (...,6)."""
    dd = np.sum(d * d, axis=-1)
    return m[..., None] * np.stack([dd - d[..., 0] * d[..., 0], -d[..., 0] * d[..., 1], -d[..., 0] * d[..., 2],
                                    dd - d[..., 1] * d[..., 1], -d[..., 1] * d[..., 2], dd - d[..., 2] * d[..., 2]], axis=-1)


def attach_payload(inertial, body, mass, at, inertia=None):
    """An inertial table (..., 25, 10) (``RobotModel.inertial()``, or a batch of them) with a rigid mass welded to ``body`` at
    the point ``at`` (3,) of the body's frame: mass, centre of mass and inertia of that body are combined by the
    parallel-axis rule about the new centre of mass.  ``inertia``: the payload's own about its centre of mass in the body's
    axes, (3,3) or xx xy xz yy yz zz (None: a point mass).  ``body``, ``mass`` and ``at`` (and ``inertia``) broadcast
    against the table's leading dimensions, so ``attach_payload(model.inertial(), b, np.array([0., 0.7, 2.5]), at)`` is a
    sweep of three robots.  Returns a new array; a robot whose payload has zero mass keeps its row's bits.  Numpy only."""
    tab = np.asarray(inertial, dtype=np.float64)
    if tab.ndim < 2 or tab.shape[-2:] != (BODIES, INERTIAL_WORDS):
        raise ValueError(f"inertial must have shape (..., {BODIES}, {INERTIAL_WORDS}), got {tab.shape}")
    body, mass, at = np.asarray(body), np.asarray(mass, dtype=np.float64), np.asarray(at, dtype=np.float64)
    if body.dtype.kind not in "iu" or np.any(body < 0) or np.any(body >= BODIES):
        raise ValueError(f"body must be an integer in 0..{BODIES - 1}")
    if not (np.all(np.isfinite(mass)) and np.all(mass >= 0.)):
        raise ValueError("the payload's mass must be finite and >= 0")
    if at.shape[-1:] != (3,) or not np.all(np.isfinite(at)):
        raise ValueError("at must be a finite point (..., 3) of the body's frame")
    own = np.zeros(6)
    if inertia is not None:
        own = np.asarray(inertia, dtype=np.float64)
        if own.shape[-2:] == (3, 3):
            own = np.stack([own[..., 0, 0], own[..., 0, 1], own[..., 0, 2], own[..., 1, 1], own[..., 1, 2], own[..., 2, 2]], axis=-1)
        if own.shape[-1:] != (6,) or not np.all(np.isfinite(own)):
            raise ValueError("inertia must be finite, (..., 3, 3) or (..., 6) = xx xy xz yy yz zz")
    lead = np.broadcast_shapes(tab.shape[:-2], body.shape, mass.shape, at.shape[:-1], own.shape[:-1])
    out = np.array(np.broadcast_to(tab, lead + tab.shape[-2:]), order='C')           # (a copy: writable, C-contiguous)
    body, mass = np.broadcast_to(body, lead), np.broadcast_to(mass, lead)
    at, own = np.broadcast_to(at, lead + (3,)), np.broadcast_to(own, lead + (6,))
    row = np.take_along_axis(out, body[..., None, None], axis=-2)[..., 0, :]      # (..., 10): the body's words
    m0, c0, I0 = row[..., 0], row[..., 1:4], row[..., 4:10]
    m = m0 + mass
    c = (m0[..., None] * c0 + mass[..., None] * at) / np.where(m > 0., m, 1.)[..., None]
    I = I0 + _parallel_axes(m0, c0 - c) + own + _parallel_axes(mass, at - c)
    new = np.where((mass > 0.)[..., None], np.concatenate([m[..., None], c, I], axis=-1), row)
    np.put_along_axis(out, body[..., None, None], new[..., None, :], axis=-2)
    return out


class BatchedRobot:
    """``RobotModel`` on the GPU: ``evaluate(q, v)`` is one launch of csrc/rbd_kernel.hpp for the whole batch.

    ``inertial``: a contiguous fp64 (B, 25, 10) tensor on the device gives every robot of the batch its own link masses,
    centres of mass and inertias (``RobotModel.inertial()`` is the model's row, ``attach_payload`` welds a load to a body);
    ``evaluate`` then launches ``cmpc_rbd_eval_inertial`` (csrc/rbd_inertial.hip), and everything that goes through it --
    ``task_model``, ``walking_model``, ``measure``, ``simulate`` -- sees the robot it describes.  The tensor is read at every
    launch and kept by reference: rewriting a row between ticks picks a box up or drops it.  A row with a non-finite word, a
    negative mass or no mass at all makes that robot's evaluation NaN.  None (the default): the shared model, as before.

    The MPC is told separately: ``BatchedRollout(mass=robot.total_mass)`` plans for the robot that is simulated, while the
    rollout's default, the scene's mass, leaves the payload unknown to the MPC -- the reference's payload experiment."""

    def __init__(self, model, device="cuda:0", g=9.81, inertial=None):
        import torch
        from . import capi
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedRobot needs a ROCm GPU: there is no CPU fallback")
        self.model, self.g = model, float(g)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = capi.load()
        self._handle = ctypes.c_void_p()
        self._tables = model.tables()                    # (kept: the pointers are read during the call only, but cheap)
        rc = self._lib.cmpc_rbd_model_create(self.device.index, *(a.ctypes.data for a in self._tables), ctypes.byref(self._handle))
        if rc != 0:
            raise ValueError(self._lib.cmpc_rbd_last_error().decode())
        self.joint_sel = None
        self._inertial = None
        self.set_inertial(inertial)

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            self._lib.cmpc_rbd_model_destroy(h)

    def set_inertial(self, t):
        """Every robot's own inertial table: a contiguous fp64 (B, 25, 10) tensor on this GPU, kept by reference and read at
        every ``evaluate`` (B must be that call's batch), or None for the shared model's."""
        import torch
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 3
                                  and tuple(t.shape[1:]) == (BODIES, INERTIAL_WORDS) and t.device == self.device):
            raise ValueError(f"inertial must be a contiguous fp64 tensor of shape (B, {BODIES}, {INERTIAL_WORDS}) on {self.device}, "
                             f"or None")
        self._inertial = t

    @property
    def inertial(self):
        """The tensor of ``set_inertial``, or None."""
        return self._inertial

    @property
    def total_mass(self):
        """The model's total mass (a float); with an inertial table a (B,) tensor, every robot's own as the kernel forms
        it: its row's masses summed in body order, at the table's present contents."""
        if self._inertial is None:
            return self.model.total_mass
        total = self._inertial[:, 0, 0].clone()
        for i in range(1, BODIES):
            total = total + self._inertial[:, i, 0]
        return total

    def evaluate(self, q, v, outputs=Evaluation._fields):
        """q, v (B,30) contiguous fp64 on this GPU -> ``Evaluation(J (B,21,30), jdqd (B,21), M (B,30,30), h (B,30), pose
        (B,21), vel (B,21), centroid (B,9))`` on the current stream.  ``outputs``: the fields wanted; the others are None
        (the kernel skips them).  With an inertial table (``set_inertial``) robot b is evaluated with row b of it."""
        import torch
        B = q.shape[0]
        for name, t in (("q", q), ("v", v)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                    and tuple(t.shape) == (B, DOFS) and t.device == self.device):
                raise ValueError(f"{name} must be a contiguous fp64 tensor of shape ({B}, {DOFS}) on {self.device}")
        if self._inertial is not None and self._inertial.shape[0] != B:
            raise ValueError(f"the inertial table holds {self._inertial.shape[0]} robots, q and v {B}")
        shapes = dict(J=(B, ROWS, DOFS), jdqd=(B, ROWS), M=(B, DOFS, DOFS), h=(B, DOFS), pose=(B, ROWS), vel=(B, ROWS),
                      centroid=(B, 9))
        unknown = set(outputs) - set(shapes)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        out = {k: (torch.empty(shapes[k], dtype=torch.float64, device=self.device) if k in outputs else None) for k in Evaluation._fields}
        if B > 0:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            ptrs = [None if out[k] is None else out[k].data_ptr() for k in Evaluation._fields]
            if self._inertial is None:
                rc = self._lib.cmpc_rbd_eval(self._handle, B, q.data_ptr(), v.data_ptr(), self.g, *ptrs, ctypes.c_void_p(stream))
            else:
                rc = self._lib.cmpc_rbd_eval_inertial(self._handle, B, q.data_ptr(), v.data_ptr(), self._inertial.data_ptr(), self.g,
                                                      *ptrs, ctypes.c_void_p(stream))
            if rc != 0:
                raise RuntimeError(self._lib.cmpc_rbd_last_error().decode())
        return Evaluation(**out)

    def task_model(self, q, v, redundant_dofs=HRP4_REDUNDANT_DOFS):
        """A callable for ``BatchedRollout.attach_whole_body_tasks(qp, model)``.  q, v: (B,30) device tensors the caller may
        update in place between ticks.  Per tick it evaluates the kernel and returns the ``solve_tasks`` inputs with
        Jdot = None and -jdqd folded into the feed-forward; the CoM rows follow the MPC's ``desired`` (com_acc,
        com_pos - pose, com_vel - vel), every other error and feed-forward is zero (the robot holds its pose), and
        joint_selection is that of ``redundant_dofs``.  ``last_evaluation`` keeps the tick's kernel outputs."""
        import torch
        sel = torch.from_numpy(self.model.joint_selection(redundant_dofs)).to(self.device)
        nacc = ROWS + DOFS

        def model(rollout, desired):
            ev = self.evaluate(q, v)
            model.last_evaluation = ev
            B = q.shape[0]
            ff = torch.zeros((B, nacc), dtype=torch.float64, device=self.device)
            pe = torch.zeros((B, nacc), dtype=torch.float64, device=self.device)
            ve = torch.zeros((B, nacc), dtype=torch.float64, device=self.device)
            ff[:, :ROWS] = -ev.jdqd
            ff[:, 12:15] += desired["com_acc"]
            pe[:, 12:15] = desired["com_pos"] - ev.pose[:, 12:15]
            ve[:, 12:15] = desired["com_vel"] - ev.vel[:, 12:15]
            return ev.J, None, ff, pe, ve, None, ev.M, ev.h, sel

        model.last_evaluation = None
        return model

    # ---- the walking loop (include/cmpc_walk.h) ----------------------------------------------------------------------------
    def _checked(self, name, t, shape, dtype=None):
        import torch
        dtype = torch.float64 if dtype is None else dtype
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)
                and t.device == self.device):
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}")
        return t

    def task_references(self, gait, t, scene_id, plan_pos, ev, com_des, q, v, q_ref=None, outputs=REFERENCE_FIELDS):
        """One launch of ``cmpc_walk_task_refs``: the ``solve_tasks`` inputs of a walking robot.  t (B,) int32 and scene_id
        (B,) int32 or None (scene 0); plan_pos (B, n_steps_max, 3), every robot's own plan; ev: an ``Evaluation`` with pose,
        vel and jdqd; com_des (B,9) = desired CoM position, velocity, acceleration; q, v (B,30); q_ref (30,) the posture the
        joint task holds (None: zeros).  Returns ``References(ff, pos_err, vel_err (B,51), feet_des (B,36))`` on the
        current stream; fields not in ``outputs`` are None (the kernel skips them)."""
        import torch
        if not isinstance(gait, Gait) or gait.device != self.device:
            raise ValueError(f"gait must be a rbd.Gait on {self.device}")
        B = q.shape[0]
        self._checked("t", t, (B,), torch.int32)
        if scene_id is not None:
            self._checked("scene_id", scene_id, (B,), torch.int32)
        self._checked("plan_pos", plan_pos, (B, gait.n_steps_max, 3))
        for name in ("pose", "vel", "jdqd"):
            self._checked("ev." + name, getattr(ev, name), (B, ROWS))
        self._checked("com_des", com_des, (B, 9))
        self._checked("q", q, (B, DOFS))
        self._checked("v", v, (B, DOFS))
        if q_ref is not None:
            self._checked("q_ref", q_ref, (DOFS,))
        unknown = set(outputs) - set(REFERENCE_FIELDS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        out = {k: (torch.empty((B, FEET_WORDS if k == "feet_des" else NACC), dtype=torch.float64, device=self.device)
                   if k in outputs else None) for k in REFERENCE_FIELDS}
        if B > 0:
            ptr = lambda x: None if x is None else x.data_ptr()
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.cmpc_walk_task_refs(gait._handle, B, t.data_ptr(), ptr(scene_id), plan_pos.data_ptr(), ev.pose.data_ptr(),
                                               ev.vel.data_ptr(), ev.jdqd.data_ptr(), com_des.data_ptr(), q.data_ptr(), v.data_ptr(),
                                               ptr(q_ref), *(ptr(out[k]) for k in REFERENCE_FIELDS), ctypes.c_void_p(stream))
            if rc != 0:
                raise RuntimeError(self._lib.cmpc_walk_last_error().decode())
        return References(**out)

    def integrate(self, q, v, qdd, dt, hold=None, out=None):
        """One launch of ``cmpc_walk_integrate``: (q, v) (B,30) advanced by dt with the acceleration qdd (B,30) in the
        body-twist convention of this module.  hold (B,) uint8 / bool: rows that keep (q, v); a row with a non-finite word
        keeps them too.  out: (q_out, v_out), which may be (q, v) themselves; None allocates.  Returns (q_out, v_out)."""
        import torch
        B = q.shape[0]
        for name, x in (("q", q), ("v", v), ("qdd", qdd)):
            self._checked(name, x, (B, DOFS))
        if hold is not None:
            if torch.is_tensor(hold) and hold.dtype == torch.bool:
                hold = hold.view(torch.uint8)                     # (same bytes: True is 1)
            self._checked("hold", hold, (B,), torch.uint8)
        q_out, v_out = (torch.empty_like(q), torch.empty_like(v)) if out is None else out
        self._checked("q_out", q_out, (B, DOFS))
        self._checked("v_out", v_out, (B, DOFS))
        if B > 0:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.cmpc_walk_integrate(self.device.index, B, q.data_ptr(), v.data_ptr(), qdd.data_ptr(), float(dt),
                                               None if hold is None else hold.data_ptr(), q_out.data_ptr(), v_out.data_ptr(),
                                               ctypes.c_void_p(stream))
            if rc != 0:
                raise RuntimeError(self._lib.cmpc_walk_last_error().decode())
        return q_out, v_out

    def measure(self, ev, state, alive=None, z_min=-np.inf, tilt_max=None, outputs=Measurement._fields):
        """One launch of ``cmpc_walk_measure``: the robot's own centroid (``ev.centroid`` (B,9): CoM, its velocity, the
        angular momentum about it) and the third angle of each foot pose (``ev.pose`` (B,21)) become words 0..8, 12 and 13
        of ``state`` (B,16), the rollout's state, in place.  A robot with ``alive[b] == 0`` (alive (B,) bool / uint8, or
        None: all alive) keeps its state; one with a non-finite word in its evaluation, with its CoM not above ``z_min`` or
        its base tilted past ``tilt_max`` (radians; None: no limit) keeps its state too and ``alive[b]`` becomes 0.
        Returns ``Measurement(x_meas (B,20), innovation (B,9))`` on the current stream: the measured x0 in the layout
        ``BatchedRollout.track`` takes, and measured minus the state's words 0..8 as they were; the rows of robots that
        were not measured are NaN, fields not in ``outputs`` are None (the kernel skips them)."""
        import torch
        B = state.shape[0]
        self._checked("ev.centroid", ev.centroid, (B, 9))
        self._checked("ev.pose", ev.pose, (B, ROWS))
        self._checked("state", state, (B, 16))
        if alive is not None:
            if torch.is_tensor(alive) and alive.dtype == torch.bool:
                alive = alive.view(torch.uint8)                   # (same bytes: True is 1, and the kernel writes 0)
            self._checked("alive", alive, (B,), torch.uint8)
        unknown = set(outputs) - set(Measurement._fields)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        cos_tilt_min = -np.inf if tilt_max is None else float(np.cos(tilt_max))
        out = {k: (torch.empty((B, 20 if k == "x_meas" else 9), dtype=torch.float64, device=self.device) if k in outputs else None)
               for k in Measurement._fields}
        ptr = lambda x: None if x is None else x.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.cmpc_walk_measure(self.device.index, B, ev.centroid.data_ptr(), ev.pose.data_ptr(), float(z_min), cos_tilt_min,
                                         state.data_ptr(), ptr(alive), ptr(out["x_meas"]), ptr(out["innovation"]),
                                         ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(self._lib.cmpc_walk_last_error().decode())
        return Measurement(**out)

    def simulate(self, q, v, ev, tau, foot_mu, plant, ext=None, hold=None, impulse=None, out=None, outputs=PLANT_OUTPUTS):
        """One launch of ``cmpc_walk_plant_step``: (q, v) (B,30) advanced by ``plant.dt`` under the joint torques ``tau``
        ((B,24), or a (B,24) view with unit stride along its rows such as ``solve_tasks``' tau; None: zero torques), the
        world-frame wrench ``ext`` (B,6) = [moment, force] on the base origin (None: none) and a flat floor with friction
        under the eight sole vertices.  ev: the ``Evaluation`` at that same (q, v) with M, h, J and pose; foot_mu (B,2):
        half foot size and the floor's friction; plant: a ``Plant``.  hold (B,) uint8 / bool: rows that keep (q, v).
        impulse (B,24): last tick's impulses as the warm start, overwritten with this tick's (None: a cold start; the
        impulses are returned in a fresh tensor if ``outputs`` names them).  out: (q_out, v_out), which may be (q, v)
        themselves; None allocates.  Returns ``PlantStep(q, v, impulse, status, residual)`` on the current stream; status
        and residual are None unless in ``outputs``."""
        import torch
        if not isinstance(plant, Plant):
            raise ValueError("plant must be a rbd.Plant")
        B = q.shape[0]
        self._checked("q", q, (B, DOFS))
        self._checked("v", v, (B, DOFS))
        self._checked("ev.M", ev.M, (B, DOFS, DOFS))
        self._checked("ev.h", ev.h, (B, DOFS))
        self._checked("ev.J", ev.J, (B, ROWS, DOFS))
        self._checked("ev.pose", ev.pose, (B, ROWS))
        tau_ld = DOFS - BASE
        if tau is not None:
            if not (torch.is_tensor(tau) and tau.is_cuda and tau.dtype == torch.float64 and tuple(tau.shape) == (B, DOFS - BASE)
                    and tau.device == self.device and (B == 0 or tau.stride(1) == 1) and (B <= 1 or tau.stride(0) >= DOFS - BASE)):
                raise ValueError(f"tau must be a fp64 tensor of shape ({B}, {DOFS - BASE}) on {self.device} with unit stride "
                                 f"along its rows and a row stride >= {DOFS - BASE}")
            tau_ld = tau.stride(0) if B > 1 else DOFS - BASE
        self._checked("foot_mu", foot_mu, (B, 2))
        if ext is not None:
            self._checked("ext", ext, (B, 6))
        if hold is not None:
            if torch.is_tensor(hold) and hold.dtype == torch.bool:
                hold = hold.view(torch.uint8)                     # (same bytes: True is 1)
            self._checked("hold", hold, (B,), torch.uint8)
        unknown = set(outputs) - set(PLANT_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        if impulse is not None:
            self._checked("impulse", impulse, (B, IMPULSE_WORDS))
        elif "impulse" in outputs:
            impulse = torch.zeros((B, IMPULSE_WORDS), dtype=torch.float64, device=self.device)
        q_out, v_out = (torch.empty_like(q), torch.empty_like(v)) if out is None else out
        self._checked("q_out", q_out, (B, DOFS))
        self._checked("v_out", v_out, (B, DOFS))
        status = torch.empty((B,), dtype=torch.int32, device=self.device) if "status" in outputs else None
        residual = torch.empty((B,), dtype=torch.float64, device=self.device) if "residual" in outputs else None
        if B > 0:
            ptr = lambda x: None if x is None else x.data_ptr()
            prm = plant.params()
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.cmpc_walk_plant_step(self.device.index, B, q.data_ptr(), v.data_ptr(), ev.M.data_ptr(), ev.h.data_ptr(),
                                                ev.J.data_ptr(), ev.pose.data_ptr(), ptr(tau), tau_ld, ptr(ext), foot_mu.data_ptr(),
                                                ptr(hold), ctypes.byref(prm), ptr(impulse), q_out.data_ptr(), v_out.data_ptr(),
                                                ptr(status), ptr(residual), ctypes.c_void_p(stream))
            if rc != 0:
                raise RuntimeError(self._lib.cmpc_walk_last_error().decode())
        return PlantStep(q_out, v_out, impulse, status, residual)

    def walking_model(self, q, v, gait, q_ref=None, integrate=True, redundant_dofs=HRP4_REDUNDANT_DOFS, fall=None, plant=None,
                      foot_mu=None, ext=None):
        """A callable for ``BatchedRollout.attach_whole_body_tasks(qp, model)`` that walks: per tick it evaluates the
        kernel at (q, v), forms every task reference from the robot's own adapted plan (``task_references`` on the
        rollout's ``t``, ``scene_id`` and ``plan_pos``, the CoM rows from the MPC's ``desired``) and returns the
        ``solve_tasks`` inputs.  Its ``advance(rollout, last_wbc)``, which the rollout calls after the QP, integrates
        q, v in place by the QP's acceleration with dt = the spec's delta; a robot whose QP failed or that is no
        longer alive holds.  q_ref (30,): the posture of the joint task (None: the first robot's q now).
        ``integrate=False`` leaves q, v to the caller.  ``last_evaluation`` and ``last_references`` keep the tick's.
        Its ``measure(rollout)``, with which a rollout built with ``feedback=True`` begins its tick, evaluates (q, v) and
        launches ``measure`` on the rollout's ``state`` and ``alive`` (fall = (z_min, tilt_max): the guards of ``measure``);
        the result is kept as ``last_measurement``, and the same tick's ``model(rollout, desired)`` uses that evaluation
        instead of launching a second one.
        With ``plant`` (a ``Plant``) ``advance`` launches ``simulate`` instead of ``integrate``: the tick's evaluation, the
        QP's torques, the wrench ``ext`` ((B,6), which the caller may rewrite between ticks: that is how a fleet is pushed)
        and the floor move the robot, with hold = not alive.  A robot whose QP failed is not held: it receives the zeros
        the QP returned and goes limp under gravity.  foot_mu (B,2): half foot size and the floor's friction (None: 0.05
        and the rollout's ``state[:, 15]`` at the first tick).  ``impulse`` (B,24) carries the warm start from tick to tick
        and ``last_plant`` keeps the tick's ``PlantStep``."""
        import torch
        sel = torch.from_numpy(self.model.joint_selection(redundant_dofs)).to(self.device)
        q_ref = q[0].clone() if q_ref is None else q_ref
        z_min, tilt_max = (-np.inf, None) if fall is None else fall
        if plant is not None and not isinstance(plant, Plant):
            raise ValueError("plant must be a rbd.Plant or None")
        if plant is None and (foot_mu is not None or ext is not None):
            raise ValueError("foot_mu and ext go with a plant")
        B = q.shape[0]
        if foot_mu is not None:
            self._checked("foot_mu", foot_mu, (B, 2))
        if ext is not None:
            self._checked("ext", ext, (B, 6))
        floor = [foot_mu]
        measured = []                                             # the evaluation of a tick that began with measure()

        def measure(rollout):
            ev = self.evaluate(q, v)
            model.last_measurement = self.measure(ev, rollout.state, rollout.alive, z_min=z_min, tilt_max=tilt_max)
            measured[:] = [ev]
            return model.last_measurement

        def model(rollout, desired):
            ev = measured.pop() if measured else self.evaluate(q, v)
            com_des = torch.cat([desired["com_pos"], desired["com_vel"], desired["com_acc"]], dim=1).contiguous()
            refs = self.task_references(gait, rollout.t, getattr(rollout, "scene_id", None), rollout.plan_pos, ev, com_des, q, v, q_ref)
            model.last_evaluation, model.last_references = ev, refs
            return ev.J, None, refs.ff, refs.pos_err, refs.vel_err, None, ev.M, ev.h, sel

        def advance(rollout, last_wbc):
            hold = (last_wbc[3] != 0) | ~rollout.alive
            self.integrate(q, v, last_wbc[1], rollout.spec.delta, hold=hold, out=(q, v))

        def simulate(rollout, last_wbc):
            if floor[0] is None:
                floor[0] = torch.stack([torch.full_like(rollout.state[:, 15], 0.05), rollout.state[:, 15]], dim=1).contiguous()
            ev = model.last_evaluation                           # the tick's own: (q, v) have not moved since
            model.last_plant = self.simulate(q, v, ev, last_wbc[0], floor[0], plant, ext=ext, hold=~rollout.alive,
                                             impulse=model.impulse, out=(q, v))

        model.last_evaluation = model.last_references = model.last_measurement = None
        model.measure = measure
        if plant is not None:
            model.impulse = torch.zeros((B, IMPULSE_WORDS), dtype=torch.float64, device=self.device)
            model.last_plant = None
            model.ext = ext
        if integrate:
            model.advance = advance if plant is None else simulate
        return model


class Gait:
    """The gait tables of a ``workloads.Scene`` or ``SceneSet`` on the GPU (``cmpc_walk_gait_create``): what
    ``BatchedRobot.task_references`` reads of the walk besides every robot's own plan positions.  ``tables``: the dict of
    ``gait_tables()`` instead of a scene.  A malformed table is refused with the native validation's message."""

    def __init__(self, scene_or_set=None, device="cuda:0", tables=None):
        import torch
        from . import capi
        if not torch.cuda.is_available():
            raise RuntimeError("Gait needs a ROCm GPU: there is no CPU fallback")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if (scene_or_set is None) == (tables is None):
            raise ValueError("Gait takes a Scene or SceneSet, or the dict of its gait_tables(), not both")
        self.tables = gait_arguments(scene_or_set.gait_tables() if tables is None else tables)
        self.S, self.T_max, self.n_steps_max = self.tables[:3]
        self._lib = capi.load()
        self._handle = ctypes.c_void_p()
        rc = self._lib.cmpc_walk_gait_create(self.device.index, *(a.ctypes.data if isinstance(a, np.ndarray) else a for a in self.tables),
                                             ctypes.byref(self._handle))
        if rc != 0:
            raise ValueError(self._lib.cmpc_walk_last_error().decode())

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            self._lib.cmpc_walk_gait_destroy(h)


def gait_arguments(tab):
    """The dict of ``gait_tables()`` as the arguments of ``cmpc_walk_gait_create`` after the device: (S, T_max,
    n_steps_max, T, step_idx, n_steps, step_start, ss_dur, support_l, ang, init_feet, step_height, delta), the arrays
    contiguous in the ABI's types.  Shapes are checked here; the values by the native validation."""
    T = np.ascontiguousarray(tab['T'], dtype=np.int32)
    step_idx = np.ascontiguousarray(tab['step_idx'], dtype=np.int32)
    step_start = np.ascontiguousarray(tab['step_start'], dtype=np.int32)
    if T.ndim != 1 or step_idx.ndim != 2 or step_start.ndim != 2:
        raise ValueError("gait tables: T (S,), step_idx (S, T_max), step_start (S, n_steps_max)")
    S, Tm, nm = T.shape[0], step_idx.shape[1], step_start.shape[1]
    arrays = (T, step_idx, np.ascontiguousarray(tab['n_steps'], dtype=np.int32), step_start,
              np.ascontiguousarray(tab['ss_dur'], dtype=np.int32), np.ascontiguousarray(tab['support_l'], dtype=np.uint8),
              np.ascontiguousarray(tab['ang'], dtype=np.float64), np.ascontiguousarray(tab['init_feet'], dtype=np.float64))
    for a, shape, name in zip(arrays, ((S,), (S, Tm), (S,), (S, nm), (S, nm), (S, nm), (S, nm, 3), (S, 12)),
                              ('T', 'step_idx', 'n_steps', 'step_start', 'ss_dur', 'support_l', 'ang', 'init_feet')):
        if a.shape != shape:
            raise ValueError(f"gait tables: {name} must have shape {shape}, got {a.shape}")
    return (S, Tm, nm) + arrays + (float(tab['step_height']), float(tab['delta']))
