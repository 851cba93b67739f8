"""The robot's placement at reset, on the host: the batched kinematics of one arm chain (ArmChain) and the base pose search built on it
(BasePoseSearch: Robot.position_robot_toc, robot.py:123-215, for one arm or two; Robot.ik_random_restarts from a fixed base, robot.py:84-121).
Bullet's IK is replaced by damped least squares; the search keeps the reference's structure (50 attempts, the start pose and position-only
goals, success threshold 0.03, the joint-limit-weighted kinematic isotropy as the score).  Every sampler that places an arm holds one
BasePoseSearch with its own task's defaults."""
import numpy as np

from ..model import xform as X

D = np.deg2rad


class ArmChain:
    """Batched (numpy) kinematics of the serial chain base -> end-effector link of the compiled robot."""

    def __init__(self, blob, second=False):
        """second: the chain to the second end effector (AGX_T_EE2_*: the left arm of a two-armed robot holding tool_left)"""
        self.blob = blob
        ee = blob.task_i('EE2_LINK' if second else 'EE_LINK')
        chain = []
        d = ee
        while d >= 0:
            chain.append(d)
            d = blob.robot_i(d, 'PARENT')
        self.chain = chain[::-1]                                  # root -> ee
        assert all(blob.robot_i(d, 'JTYPE') == 0 for d in self.chain)
        self.tpos = np.array([blob.robot_f(d, 'TPOS', 3) for d in self.chain])
        self.tR = np.array([X.quat_to_mat(blob.robot_f(d, 'TQUAT', 4)) for d in self.chain])
        self.axis = np.array([blob.robot_f(d, 'AXIS', 3) for d in self.chain])
        self.lower = np.array([blob.robot_f(d, 'LOWER') for d in self.chain])
        self.upper = np.array([blob.robot_f(d, 'UPPER') for d in self.chain])
        self.act = [blob.robot_i(d, 'ACT') for d in self.chain]
        assert all(a >= 0 for a in self.act), 'every joint between the base and the end effector is an arm joint'
        self.ee_pos = blob.task_f('EE2_POS' if second else 'EE_POS', 3)
        self.ee_R = X.quat_to_mat(blob.task_f('EE2_QUAT' if second else 'EE_QUAT', 4))
        self.n = len(self.chain)

    @staticmethod
    def _rot(axis, ang):
        """Rodrigues, batched over ang (B,) for one axis (3,) -> (B, 3, 3)"""
        a = axis / np.linalg.norm(axis)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        s, c = np.sin(ang)[:, None, None], np.cos(ang)[:, None, None]
        return np.eye(3)[None] + s * K[None] + (1 - c) * (K @ K)[None]

    def fk(self, base_pos, base_R, q):
        """base_pos (B,3), base_R (B,3,3), q (B,n) -> ee pos (B,3), ee R (B,3,3), joint origins (B,n,3), joint axes in world (B,n,3)"""
        B = q.shape[0]
        p, R = base_pos.copy(), base_R.copy()
        orig, axw = np.zeros((B, self.n, 3)), np.zeros((B, self.n, 3))
        for k in range(self.n):
            p = p + np.einsum('bij,j->bi', R, self.tpos[k])
            R = R @ self.tR[k][None]
            orig[:, k] = p
            axw[:, k] = np.einsum('bij,j->bi', R, self.axis[k])
            R = R @ self._rot(self.axis[k], q[:, k])
        pe = p + np.einsum('bij,j->bi', R, self.ee_pos)
        return pe, R @ self.ee_R[None], orig, axw

    def jacobian(self, pe, orig, axw):
        Jl = np.cross(axw, pe[:, None, :] - orig)                 # (B,n,3)
        return np.concatenate([Jl.transpose(0, 2, 1), axw.transpose(0, 2, 1)], axis=1)    # (B,6,n)

    def ik(self, base_pos, base_R, q0, target_pos, target_R=None, iters=100, damping=0.05, maxstep=0.5):
        """Damped least squares, batched; target_R None = position only.  Returns q (B,n)."""
        q = q0.copy()
        for _ in range(iters):
            pe, Re, orig, axw = self.fk(base_pos, base_R, q)
            J = self.jacobian(pe, orig, axw)
            e = target_pos - pe
            if target_R is not None:
                Rerr = target_R @ Re.transpose(0, 2, 1)
                w = 0.5 * np.stack([Rerr[:, 2, 1] - Rerr[:, 1, 2], Rerr[:, 0, 2] - Rerr[:, 2, 0], Rerr[:, 1, 0] - Rerr[:, 0, 1]], axis=1)
                e = np.concatenate([e, w], axis=1)
            else:
                J = J[:, :3]
            A = J @ J.transpose(0, 2, 1) + damping ** 2 * np.eye(J.shape[1])[None]
            dq = np.einsum('bji,bj->bi', J, np.linalg.solve(A, e[..., None])[..., 0])
            step = np.abs(dq).max(axis=1, keepdims=True)
            dq = np.where(step > maxstep, dq * (maxstep / np.maximum(step, 1e-30)), dq)
            q = np.clip(q + dq, self.lower[None], self.upper[None])
        return q


def mat_to_quat_batch(R):
    return np.array([X.mat_to_quat(r) for r in R])


def joint_limited_weighting(q, lower, upper):
    """Robot.joint_limited_weighting (robot.py:217-228), batched over q (B,n) -> diagonal weights (B,n)"""
    phi, lam = 0.5, 0.05
    qr = 0.5 * (upper - lower)
    w = 1.0 - np.power(phi, (qr - np.abs(qr - q + lower)) / (lam * qr) + 1)
    return np.maximum(w, 0.001)


class BasePoseSearch:
    """toc_base / ee_rpy: the task's toc_base_pos_offset and toc_ee_orient_rpy for blobs whose meta does not state them; self_guard: reject start
    poses whose arm folds into the robot's own pedestal (_arm_in_pedestal: the Sawyer); dual: a second chain (ArmChain(second=True)) for _toc_dual"""

    def __init__(self, blob, toc_base=None, ee_rpy=None, self_guard=False, dual=False):
        m = blob.meta
        self.blob, self.arm = blob, ArmChain(blob)
        self.arm2 = ArmChain(blob, second=True) if dual else None
        self.toc_base = np.array([-0.85, -0.4, 0]) + np.array(m['toc_base'] if toc_base is None else m.get('toc_base', toc_base))      # robot.py:142 + toc_base_pos_offset
        self.ee_R = X.quat_to_mat(X.quat_from_rpy(m['ee_rpy'] if ee_rpy is None else m.get('ee_rpy', ee_rpy)))                          # toc_ee_orient_rpy
        self.self_guard = self_guard

    def arm_joints(self, q_arm, q_arm2=None):
        """the robot's joint vector with the chain(s) at the given angles, everything else at zero"""
        q = np.zeros(self.blob.nrobot)
        q[self.arm.chain] = q_arm
        if q_arm2 is not None:
            q[self.arm2.chain] = q_arm2
        return q

    def tool_pose(self, base_pos, base_quat, q_arm, second=False):
        """base frame of the tool in the gripper (tool.py:49-62): end-effector frame o TOOL"""
        arm = self.arm2 if second else self.arm
        pe, Re, _, _ = arm.fk(np.asarray(base_pos)[None], X.quat_to_mat(base_quat)[None], q_arm[None])
        return X.compose(pe[0], X.mat_to_quat(Re[0]), self.blob.task_f('TOOL2_POS' if second else 'TOOL_POS', 3), self.blob.task_f('TOOL2_QUAT' if second else 'TOOL_QUAT', 4))

    def search(self, rng, start_pos, goals, tries=4, **kw):
        """_toc, drawn again (at most `tries` times) while no candidate reaches its start pose"""
        for _ in range(tries):
            res = self._toc(rng, start_pos, goals, **kw)
            if res is not None:
                return res
        raise AssertionError('no reachable base pose found')

    def search_dual(self, rng, starts, goals, tries=4):
        """_toc_dual for the two chains of this robot, drawn again like search"""
        for _ in range(tries):
            res = self._toc_dual(rng, [self.arm, self.arm2], starts, goals)
            if res is not None:
                return res
        raise AssertionError('no reachable base pose found')

    # ---- TOC base pose search (robot.py:123-215) ---------------------------------------------------------
    def _toc(self, rng, start_pos, goals, attempts=50, goal_Rs=None, right_side=True):
        """one arm.  goal_Rs: optional end-effector orientation (3x3) per goal, None = position only; right_side=False: the base is drawn on the
        human's left and turned by pi (env.py:298 base_euler_orient, robot.py:143).  Returns (base_pos, base_quat, q_arm, goals reached,
        manipulability) or None"""
        res = self._toc_dual(rng, [self.arm], [start_pos], [goals], attempts, [goal_Rs], right_side)
        return res and res[:2] + (res[2][0],) + res[3:]

    def _toc_dual(self, rng, arms, starts, goals, attempts=50, goal_Rs=None, right_side=True):
        """Robot.position_robot_toc (robot.py:123-215), for arms = ['right', 'left'] too: `attempts` random base poses, ONE for all arms; the goals
        an arm reaches and its manipulability (the joint-limit-weighted kinematic isotropy) add up over the arms, every start pose must be
        reachable.  arms: [ArmChain, ...]; starts[i]: start position of arm i (orientation self.ee_R); goals[i]: goals of arm i, position only
        unless goal_Rs[i] gives orientations.  Returns (base_pos, base_quat, [q_arm_i], goals reached, manipulability) or None."""
        A = attempts
        rp = np.stack([rng.uniform(-0.5, 0, size=A) if right_side else rng.uniform(0, 0.5, size=A), rng.uniform(-0.5, 0.5, size=A), np.zeros(A)], axis=1)     # random_position 0.5
        yaw = (0.0 if right_side else np.pi) + D(rng.uniform(-30, 30, size=A))                              # random_rotation 30
        # the reference draws position and yaw alternately per attempt; the draws here are made in two blocks (not stream compatible anyway)
        base_pos = self.toc_base[None] + rp
        base_R = np.array([X.quat_to_mat(X.quat_from_rpy([0, 0, y])) for y in yaw])
        ngoal, manip, valid = np.zeros(A), np.zeros(A), np.ones(A, dtype=bool)
        qstart = []
        for arm, start, gl, gRs in zip(arms, starts, goals, goal_Rs or [None] * len(arms)):
            lo = np.where(arm.lower < -1e9, -2 * np.pi, arm.lower)
            hi = np.where(arm.upper > 1e9, 2 * np.pi, arm.upper)
            q0 = rng.uniform(lo, hi, size=(A, 1 + len(gl), arm.n))                                           # agent.py:263 rest poses
            for g in range(1 + len(gl)):
                tp = np.repeat((start if g == 0 else gl[g - 1])[None], A, axis=0)
                gR = self.ee_R if g == 0 else (gRs[g - 1] if gRs is not None else None)
                tR = np.repeat(gR[None], A, axis=0) if gR is not None else None
                q = arm.ik(base_pos, base_R, q0[:, g], tp, tR, iters=100)                                    # max_ik_iterations=100
                pe, Re, orig, axw = arm.fk(base_pos, base_R, q)
                ok = np.linalg.norm(tp - pe, axis=1) < 0.03                                                  # robot.py:97 success_threshold
                if tR is not None:
                    qe, qt = mat_to_quat_batch(Re), X.mat_to_quat(gR)
                    ok &= np.minimum(np.linalg.norm(qe - qt[None], axis=1), np.linalg.norm(qe + qt[None], axis=1)) < 0.03
                J = arm.jacobian(pe, orig, axw)
                W = joint_limited_weighting(q, arm.lower, arm.upper)
                M = np.einsum('bij,bj,bkj->bik', J, W, J)
                det = np.maximum(np.linalg.det(M), 0)
                jl = np.power(det, 1.0 / 6) / (np.trace(M, axis1=1, axis2=2) / 6)                            # robot.py:189-191
                if g == 0:                                      # the start goal must be reachable (robot.py:196-200)
                    if self.self_guard:
                        ok &= ~self._arm_in_pedestal(base_pos, base_R, orig, pe)
                    valid &= ok
                    qstart.append(q)
                ngoal += ok
                manip += np.where(ok, jl, 0.0)
        ngoal = np.where(valid, ngoal, -1)
        manip = np.where(valid, manip, -np.inf)
        best = max(range(A), key=lambda a: (ngoal[a], manip[a]))   # first of equals = the earliest attempt, as the strict > of robot.py:204
        if ngoal[best] <= 0:
            return None
        return base_pos[best], X.mat_to_quat(base_R[best]), [q[best] for q in qstart], int(ngoal[best]), float(manip[best])

    def _arm_in_pedestal(self, base_pos, base_R, orig, pe, margin=0.09):
        """start poses whose arm folds into the robot's own pedestal (boxes of the base colliders grown by a link radius): Bullet's
        null-space IK with rest poses does not produce those elbow-down solutions, the damped least squares here can"""
        if not hasattr(self, '_ped'):
            r = self.blob.meta['ranges']['robot_base']
            self._ped = np.array([[self.blob.collider(c)['verts'].min(0) - margin, self.blob.collider(c)['verts'].max(0) + margin] for c in range(*r)])
        pts = np.concatenate([orig[:, 2:], 0.5 * (orig[:, 2:-1] + orig[:, 3:]), pe[:, None]], axis=1)          # joint origins past the shoulder, midpoints, ee
        loc = np.einsum('bji,bkj->bki', base_R, pts - base_pos[:, None])
        inside = (loc[:, :, None, :] >= self._ped[None, None, :, 0]) & (loc[:, :, None, :] <= self._ped[None, None, :, 1])
        return inside.all(-1).any(-1).any(-1)

    # ---- wheelchair-mounted robots: IK with random restarts from a fixed base (robot.py:84-121) ------------------------------------
    def _near_human(self, hm, hpos, hquat, hbase, pts, margin=0.07):
        """pts (B, K, 3): is any point closer than `margin` (an arm link's radius + clearance) to a capsule / sphere of the human?  The
        stand-in for `get_closest_points(human, distance=0)` inside ik_random_restarts (robot.py:103-108) on the host."""
        hit = np.zeros(pts.shape[0], dtype=bool)
        for link, kind, data in hm.colliders():
            lp, lq = (hbase, np.array([0, 0, 0, 1.0])) if link < 0 else (hpos[link], hquat[link])
            if kind == 'capsule':
                a, b = X.apply(lp, lq, np.stack([data[0], data[1]]))
                r = data[2]
            elif kind == 'sphere':
                a = b = X.apply(lp, lq, data[0][None])[0]
                r = data[1]
            else:
                continue
            ab = b - a
            t = np.clip(((pts - a) @ ab) / max(float(ab @ ab), 1e-12), 0, 1)
            d = np.linalg.norm(pts - (a + t[..., None] * ab), axis=-1) - r
            hit |= (d < margin).any(axis=1)
        return hit

    def _mounted_ik(self, rng, target_pos, base_pos, base_quat, human=None, restarts=64, rounds=4):
        """Robot.ik_random_restarts (robot.py:84-121) from the fixed base: random rest poses until the end effector is within 0.01 of the
        target pose and the arm is clear of the human; `restarts` of them are solved at once, the first that qualifies is taken; when
        none does, the closest one (robot.py:117-121)"""
        arm = self.arm
        bp = np.repeat(np.asarray(base_pos, dtype=np.float64)[None], restarts, axis=0)
        bR = np.repeat(X.quat_to_mat(base_quat)[None], restarts, axis=0)
        lo = np.where(arm.lower < -1e9, -2 * np.pi, arm.lower)
        hi = np.where(arm.upper > 1e9, 2 * np.pi, arm.upper)
        tp, tR = np.repeat(target_pos[None], restarts, axis=0), np.repeat(self.ee_R[None], restarts, axis=0)
        qt = X.mat_to_quat(self.ee_R)
        best = None
        for _ in range(rounds):
            q = arm.ik(bp, bR, rng.uniform(lo, hi, size=(restarts, arm.n)), tp, tR, iters=200)
            pe, Re, orig, _ = arm.fk(bp, bR, q)
            qe = mat_to_quat_batch(Re)
            err = np.linalg.norm(tp - pe, axis=1) + np.minimum(np.linalg.norm(qe - qt[None], axis=1), np.linalg.norm(qe + qt[None], axis=1))
            ok = (np.linalg.norm(tp - pe, axis=1) < 0.01) & (np.minimum(np.linalg.norm(qe - qt[None], axis=1), np.linalg.norm(qe + qt[None], axis=1)) < 0.01)
            if human is not None and ok.any():
                pts = np.concatenate([orig[:, 1:], 0.5 * (orig[:, 1:-1] + orig[:, 2:]), pe[:, None], 0.5 * (orig[:, -1:] + pe[:, None])], axis=1)
                ok &= ~self._near_human(*human, pts)
            k = int(np.argmax(ok)) if ok.any() else int(np.argmin(err))
            if best is None or err[k] < best[0]:
                best = (float(err[k]), q[k].copy(), bool(ok[k]))
            if ok.any():
                break
        return np.asarray(base_pos, dtype=np.float64).copy(), np.asarray(base_quat, dtype=np.float64), best[1], 1 if best[2] else 0, 0.0
