"""Small synthetic link trees for the dynamics phase of the substep (csrc/agx_dyn.h: kinematics, the articulated-body pass, the columns of
M^-1, the unconstrained velocity update; csrc/agx_env.h: integrate): random link records spliced into a shipped blob in place of its robot's
and its person's, every motor, limit, pair row and the tool constraint switched off, a deliberately plain float64 reference of what the
joint accelerations ARE (written from the definitions -- link Jacobians at the centres of mass, Lagrange's equations, a dense inverse -- with no
spatial algebra: not from agx_dyn.h and not from oracle/), and the comparison the emulator and the device tests judge by.

  splice / scene_blob          the blob: link records of both genders, free-body mass / inertia / gravity, parameters; the isolation recipe
  fk / jacobians / mass_matrix forward kinematics as include/agx_blob.h states the record's meaning; M = sum m Jv'Jv + Jw' I_w Jw
  velocity_products            the velocity-product terms of Lagrange's equations by the complex step on fk
  joint_dynamics / reference   gravity, velocity damping, joint damping; M^-1 per block, qdd = M^-1 (-h), frozen DoFs struck out; free_dynamics: the free bodies' substep
  point_terms                  e, eq: what the kernel's one reference point costs the entries of the links far from it (LIMITS)
  iterate                      several substeps of the reference (dy_chain, dy_tree: four)
  measures / limits            S and D32 per environment and quantity, from the reference alone
  result_of / judge / say      a debug record and the stored state against the stored values: ALL environments of a scene, maxima

WHAT IS COMPUTED.  A link's frame is its parent's frame (the robot base for parent -1, the person's base body for -2), then TPOS / TQUAT,
then a rotation about AXIS by q (JTYPE 0) or a translation along AXIS by q (JTYPE 1); TQUAT and AXIS are normalised in float64.  c_l = the
link's centre of mass COM in the world, I_l its inertia about c_l turned into the world.  Jv_l, Jw_l: the velocity of c_l and the angular
velocity of link l as linear maps of qd (column k: a_k x (c_l - p_k) and a_k for a revolute ancestor k, a_k and 0 for a prismatic one).
M = sum_l m_l Jv_l' Jv_l + Jw_l' I_l Jw_l.  h = C + G + D with
  C_k = sum_ij (dM_kj/dq_i - 1/2 dM_ij/dq_k) qd_i qd_j = (d/dq along qd of M qd)_k - d/dq_k (1/2 qd' M qd)     the derivatives by the complex step,
  G = -sum_l Jv_l' m_l g_l z           g_l: HUMAN_GRAVITY_Z for KIND bit 0, ROBOT_GRAVITY_Z otherwise
  D = -sum_l (Jv_l' F_l + Jw_l' t_l) + JDAMP qd       F_l = -m_l (k_l + k_l |v_l|) v_l, t_l = -(k_a + k_a |w_l|) I_l w_l
and qdd = M^-1 (-h) per block (robot DoFs, person DoFs: no link of one hangs on the other).  A frozen DoF d (state word `frozen`, DoFs below
32) has qdd_d = 0, row and column d of M^-1 zero, the rest the inverse of M with d struck out; its velocity stays in h.  A joint whose
own row of M is zero (nothing with mass hangs on it) counts as frozen: the kernel's documented `D > 1e-30` rule.
Free bodies (restated from predict_velocities and integrate): v' = v + dt (g z - (k_l + k_l |v|) v); w' = w + dt (I_w^-1 (-w x I_w w) -
(k_a + k_a |w|) w) with I_w = R diag(I) R', a principal moment of 0 meaning no response about that axis; x' = x + dt v'; q' = dq q
normalised, dq = (w'/|w'| sin(|w'| dt / 2), cos(|w'| dt / 2)), or (dt w' / 2, 1) where |w'| dt <= 1e-12.

LIMITS (derived from the reference alone; never from the emulator or the device).  Per environment and quantity
  S      the largest change of the reference's own result over SENS_TRIALS draws in which every input the device reads as float32 -- link
         data, parameters, q, qd, the two base poses, the free bodies' data and state -- moves one float32 ulp up or down (exact zeros stay)
  D32    the deviation of the same reference evaluated in float32 (complex64 for the step) from its float64 result
  limit  4 max(S, D32) (+ e_a e_b for entry (a, b) of M^-1, + eq_a for qdd_a: below), at least FLOOR_ULPS float32 ulps of the quantity's scale;
         a pose whose 4 max(S, D32) would reach CAP x scale is not stored.
Scales: the block's largest |M^-1| entry, the block's largest |qdd|; per free body the largest |coordinate| of its position, 1 for its
quaternion, its largest |v'| and |w'| component.  CAP is the bound tests/test_gpu_parity.py::test_debug_internals_match_oracle holds.
  e      (RAISED over the two measures the suite was proposed with, with this rounding argument; found on the emulator on dy_chain: the last
         link's diagonal entry of M^-1 at 1.4 times 4 max(S, D32), 1.1e-5 of the block's largest entry.)  The kernel refers every spatial
         quantity to one reference point r, the origin of link EE_LINK, and forms a link's inertia about r from separate float32 terms:
         I_l + m_l (|c|^2 1 - c c'), m_l [c]x, m_l 1 with c = c_l - r.  In the quadratic form of two unit joint velocities k, j (twists
         (w_k, v_k) at r) these terms are as large as |I_l| |w_k| |w_j| + m_l g_lk g_lj with g_lk = |w_k x c| + |v_k|, and cancel down to the
         link's own m_l Jv_k.Jv_j + Jw_k.I_l Jw_j, which is orders of magnitude smaller for a light link far from r.  POINT_ROUNDINGS
         roundings of at most half an ulp on each (three in forming an entry: the products, their difference, the sum with I_l; two in the
         product with the joint's twist; one in the sum over the subtree).  The roundings of different links, entries and steps are independent
         of one another, so their variances add, (half an ulp)^2 / 3 each (uniform over half an ulp either way): entry (k, j) of M carries a standard
         deviation of at most V_kj^(1/2), V_kj = POINT_ROUNDINGS / 3 x 2^-48 sum_l [...]^2 over the links both joints move, and to first order entry (a, b) of M^-1 one of
         s_ab = (sum_kj (M^-1_ak)^2 V_kj (M^-1_jb)^2)^(1/2).  V is positive semi-definite (a sum of entrywise squares of positive
         semi-definite matrices), so s_ab^2 <= s_aa s_bb: with e_a = (SIGMAS s_aa)^(1/2) the limit of entry (a, b) is 4 max(S, D32) + e_a e_b,
         SIGMAS standard deviations, the factor the limits take over S and D32 too (the terms' sizes are upper bounds -- triangle
         inequalities, the top of each binade -- so the margin is larger than the count says).  (A first version summed the terms' sizes linearly, the worst case: that put
         most limits of qdd back on the cap and was withdrawn.)  It is the conditioning of the float32 formulation about r, not of the
         problem (S), and it stays with the entries of the links far from r.
         The same roundings reach qdd = M^-1 (-h) through dM and through h, whose link terms about r -- w x (I w + c x m v_c) + v_o x m v_c,
         w x m v_c, tau + c x f, f, and the articulated inertia times the velocity-product acceleration |w_parent| |qd_d| of joint d's twist --
         cancel in the same way (found on the emulator on dy_tree: DoF 8, a second root, at 1.06 of 4 max(S, D32)): in quadrature again,
         eq_a = SIGMAS (sum_k (M^-1_ak)^2 (sum_j V_kj qdd_j^2 + Vh_k))^(1/2), Vh_k = POINT_ROUNDINGS / 3 x 2^-48 times the sum of the squares of those
         terms' sizes over the links joint k moves; the limit of qdd_a is 4 max(S, D32) + eq_a.
         Where a raised limit exceeds CAP x scale, the cap holds: no entry is ever judged more loosely than the suite judged it before.
The stored state: qd' is qd + dt qdd_device (float64) to half a float32 ulp of the sum and half an ulp of the product dt qdd_device (the
compiler may contract the update, which drops the second); where nothing cancels that is the one ulp of the sum; q' likewise from the device's own qd'."""
import json
import os

import numpy as np

from assistive_gym_amd.model import compiler as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dynamics_cases.npz')
SENS_TRIALS = 6
FLOOR_ULPS = 4.0
CAP = 1e-4
STEP = 1e-20                # the complex step: no subtraction, so any step whose square vanishes next to 1 serves (tests: 1e-30 agrees to 1e-9)
SMALL_ANGLE = 1e-12
POINT_ROUNDINGS = 6.0       # independent half-ulp roundings a link's inertia about the reference point carries into M: see e under LIMITS
SIGMAS = 4.0                # the factor the limits take over a measure (4 max(S, D32)), taken over the root-sum-square of those roundings as well
DEAD_ROW = 1e-30            # a joint whose diagonal entry of M is not above this carries nothing: frozen
# columns of a scene's `links` array (float32 [2 genders, ndof, LINK_COLS])
LK = dict(parent=0, jtype=1, kind=2, tpos=3, tquat=6, axis=10, com=13, mass=16, inertia=17, jdamp=23)
LINK_COLS = 24
FB = dict(mass=0, inertia=1, gravity=4)      # columns of `freeb` (float32 [nfree, 5])
QUANT = ('minv_r', 'minv_h', 'qdd_r', 'qdd_h')      # the columns of a scene's `lim` (float64 [poses, 4]: robot block, person block); `flim`: [poses, nfree, 4] = x, quat, v, w
PARAMS = ('DT', 'LIN_DAMP', 'ANG_DAMP', 'ROBOT_GRAVITY_Z', 'HUMAN_GRAVITY_Z')


# ---------------------------------------------------------------------------------------------------- the blob
def splice(blob, links, freeb=None, params=None):
    """`blob` with the link records overwritten from `links` (float32 [2, ndof, LINK_COLS]: gender 0 and gender 1; robot DoFs are read from
    gender 0), free-body MASS / INERTIA / GRAVITY from `freeb`, PARAMS entries from `params`, and the isolation recipe applied: MAXF = 0 and
    HAS_LIMIT = 0 in every link record, NGROUP = 0, TOOL_MAXF = 0, the person's LOWER / UPPER wide.  Only data words change."""
    from assistive_gym_amd.blob import ModelBlob
    w = blob.words.copy()
    wi, wf = w.view(np.int32), w.view(np.float32)
    h, n, nr = blob.h, blob.ndof, blob.nrobot
    links = np.asarray(links, dtype=np.float32)
    assert links.shape == (2, n, LINK_COLS)
    for g in range(2):
        for d in range(n):
            if d < nr and g == 1:
                continue
            r = links[g, d]
            o = h['OFF_ROBOT'] + blob.rec(d, g) * L.R['STRIDE']
            par = int(r[LK['parent']])
            assert par < d, 'a parent\'s index is below its child\'s'
            assert (par == -1 or 0 <= par < nr) if d < nr else (par == -2 or nr <= par < n), 'a link hangs inside its own block'
            wi[o + L.R['PARENT']], wi[o + L.R['JTYPE']] = par, int(r[LK['jtype']])
            wi[o + L.R['KIND']] = (wi[o + L.R['KIND']] & ~1) | (int(r[LK['kind']]) & 1)
            for key, col, cnt in (('TPOS', 'tpos', 3), ('TQUAT', 'tquat', 4), ('AXIS', 'axis', 3), ('COM', 'com', 3), ('MASS', 'mass', 1), ('INERTIA', 'inertia', 6), ('JDAMP', 'jdamp', 1)):
                wf[o + L.R[key]:o + L.R[key] + cnt] = r[LK[col]:LK[col] + cnt]
            wf[o + L.R['MAXF']], wi[o + L.R['HAS_LIMIT']] = 0.0, 0
            if d >= nr:
                wf[o + L.R['LOWER']], wf[o + L.R['UPPER']] = -1e6, 1e6
    if freeb is not None and blob.nfree:
        freeb = np.asarray(freeb, dtype=np.float32)
        assert freeb.shape == (blob.nfree, 5)
        for b in range(blob.nfree):
            o = h['OFF_FREE'] + b * L.F['STRIDE']
            wf[o + L.F['MASS']], wf[o + L.F['GRAVITY']] = freeb[b, FB['mass']], freeb[b, FB['gravity']]
            wf[o + L.F['INERTIA']:o + L.F['INERTIA'] + 3] = freeb[b, FB['inertia']:FB['inertia'] + 3]
    for k, v in (params or {}).items():
        assert k in PARAMS
        wf[h['OFF_PARAMS'] + L.P[k]] = np.float32(v)
    wi[L.H['NGROUP']] = 0
    wf[h['OFF_TASK'] + L.T['TOOL_MAXF']] = 0.0
    out = ModelBlob(w, blob.meta)
    from assistive_gym_amd import variants
    v = variants.pick(out)
    assert v is not None and nr <= v.max_block and blob.nhdof <= v.max_block, 'every block fits max_block'
    assert 0 <= out.task_i('EE_LINK') < n, 'EE_LINK stays a valid link'
    return out


def blob_links(blob):
    """the link records of a blob in the layout of `links` (what a scene that keeps the model's own tree starts from)"""
    out = np.zeros((2, blob.ndof, LINK_COLS), dtype=np.float32)
    for g in range(2):
        for d in range(blob.ndof):
            r = out[g, d]
            r[LK['parent']], r[LK['jtype']], r[LK['kind']] = blob.robot_i(d, 'PARENT', g), blob.robot_i(d, 'JTYPE', g), blob.robot_i(d, 'KIND', g) & 1
            for key, col, cnt in (('TPOS', 'tpos', 3), ('TQUAT', 'tquat', 4), ('AXIS', 'axis', 3), ('COM', 'com', 3), ('INERTIA', 'inertia', 6)):
                r[LK[col]:LK[col] + cnt] = blob.robot_f(d, key, cnt, g)
            r[LK['mass']], r[LK['jdamp']] = blob.robot_f(d, 'MASS', 1, g), blob.robot_f(d, 'JDAMP', 1, g)
    return out


def params(blob):
    p = {k: np.float32(blob.f[blob.h['OFF_PARAMS'] + L.P[k]]) for k in PARAMS}
    p['DT'] = np.float32(p['DT'] / np.float32(max(1, blob.h['SIM_SUBSTEPS'])))      # the substep, as the kernel forms it
    return p


# ---------------------------------------------------------------------------------------------------- the reference
def _cplx(T):
    return np.complex128 if T == np.float64 else np.complex64


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def quat_mat(q, T=np.float64):
    """rotation matrix of the quaternion (x, y, z, w), normalised; [..., 4] -> [..., 3, 3]"""
    q = np.asarray(q, dtype=T)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def axis_rot(a, th):
    """rotation about the unit axis a [3] by the angles th [B] (real or complex): Rodrigues' formula, [B, 3, 3]"""
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=a.dtype)
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    return c * np.eye(3, dtype=a.dtype) + s * K + (1 - c) * np.outer(a, a)


def model_of(links, freeb, par, nrobot, T=np.float64):
    """the numbers the reference works on, in arithmetic T: links float [ndof, LINK_COLS] of ONE gender"""
    lk = np.asarray(links)
    n = len(lk)
    f = lambda col, cnt: np.asarray(lk[:, LK[col]:LK[col] + cnt], dtype=T)
    ax = f('axis', 3)
    I6 = f('inertia', 6)
    Il = np.stack([I6[:, 0], I6[:, 3], I6[:, 4], I6[:, 3], I6[:, 1], I6[:, 5], I6[:, 4], I6[:, 5], I6[:, 2]], -1).reshape(n, 3, 3)
    parent = lk[:, LK['parent']].astype(int)
    anc = np.zeros((n, n), dtype=T)      # anc[l, k] = 1: joint k moves link l
    for l in range(n):
        k = l
        while k >= 0:
            anc[l, k] = 1
            k = parent[k]
    m = dict(T=T, n=n, nrobot=nrobot, parent=parent, rev=np.asarray(lk[:, LK['jtype']] == 0, dtype=T), anc=anc, tpos=f('tpos', 3), Rt=quat_mat(f('tquat', 4), T),
             axis=ax / np.sqrt((ax * ax).sum(1, keepdims=True)), com=f('com', 3), mass=f('mass', 1)[:, 0], Il=Il, jdamp=f('jdamp', 1)[:, 0],
             human=(lk[:, LK['kind']].astype(int) & 1) == 1, freeb=None if freeb is None else np.asarray(freeb, dtype=T))
    m.update({k: T(par[k]) for k in PARAMS})
    return m


def fk(m, q, base, hbase):
    """link frames: q [B, ndof] (real or complex), base and hbase [7] (position, quaternion xyzw) -> origins [B, ndof, 3], rotations [B, ndof, 3, 3]"""
    T, n, B = m['T'], m['n'], len(q)
    roots = {-1: (np.asarray(base[:3], dtype=T)[None], quat_mat(base[3:7], T)[None]), -2: (np.asarray(hbase[:3], dtype=T)[None], quat_mat(hbase[3:7], T)[None])}
    P, R = [], []
    for d in range(n):
        pp, PR = roots[m['parent'][d]] if m['parent'][d] < 0 else (P[m['parent'][d]], R[m['parent'][d]])
        Rd = PR @ m['Rt'][d]
        pd = PR @ m['tpos'][d] + pp
        if m['rev'][d]:
            Rd = Rd @ axis_rot(m['axis'][d], q[:, d])
        else:
            pd = pd + q[:, d, None] * (Rd @ m['axis'][d])
        P.append(np.broadcast_to(pd, (B, 3)).astype(q.dtype))
        R.append(np.broadcast_to(Rd, (B, 3, 3)).astype(q.dtype))
    return np.stack(P, 1), np.stack(R, 1)


def jacobians(m, P, R, com_scale=1.0):
    """(Jv [B, link, joint, 3], Jw likewise, world inertia [B, link, 3, 3], world centres of mass [B, link, 3]); com_scale: 1, or per link
    0 to place its mass at the link frame's origin (a planted error)"""
    aw = np.einsum('bdij,dj->bdi', R, m['axis'])
    cw = np.einsum('bdij,dj->bdi', R, m['com'] * np.asarray(com_scale, dtype=m['T']).reshape(-1, 1)) + P
    r = cw[:, :, None, :] - P[:, None, :, :]
    rev = m['rev'][None, None, :, None]
    Jv = (rev * _cross(aw[:, None, :, :], r) + (1 - rev) * aw[:, None, :, :]) * m['anc'][None, :, :, None]
    Jw = np.broadcast_to(aw[:, None, :, :], Jv.shape) * (m['anc'] * m['rev'][None, :])[None, :, :, None]
    Iw = np.einsum('bdij,djk,bdlk->bdil', R, m['Il'], R)
    return Jv, Jw, Iw, cw


def mass_matrix(m, Jv, Jw, Iw):
    return np.einsum('d,bdki,bdli->bkl', m['mass'], Jv, Jv) + np.einsum('bdki,bdij,bdlj->bkl', Jw, Iw, Jw)


def _flag_scale(m, flaws, word):
    """per link 1, or 0 where the planted error `word` (every link) or `word:d` (link d) applies"""
    s = np.ones(m['n'], dtype=m['T'])
    for f in flaws:
        if f == word:
            s[:] = 0
        elif f.startswith(word + ':'):
            s[int(f.split(':')[1])] = 0
    return s


def _com_scale(m, flaws):
    return _flag_scale(m, flaws, 'com_inertia')


def _momentum_energy(m, q, qd, base, hbase, flaws):
    """(M qd [B, ndof], qd' M qd / 2 [B]) at the poses q [B, ndof], from the links' velocities"""
    P, R = fk(m, q, base, hbase)
    Jv, Jw, Iw, _ = jacobians(m, P, R, _com_scale(m, flaws))
    v, w = np.einsum('bdki,k->bdi', Jv, qd), np.einsum('bdki,k->bdi', Jw, qd)
    Lw = np.einsum('bdij,bdj->bdi', Iw, w)
    mom = np.einsum('d,bdki,bdi->bk', m['mass'], Jv, v) + np.einsum('bdki,bdi->bk', Jw, Lw)
    return mom, ((m['mass'][None, :, None] * v * v).sum((1, 2)) + (w * Lw).sum((1, 2))) / 2


def velocity_products(m, q, qd, base, hbase, step=STEP, flaws=()):
    """C_k = sum_ij (dM_kj/dq_i - 1/2 dM_ij/dq_k) qd_i qd_j: the complex step along qd on M qd, and along every q_k on the kinetic energy"""
    T, n = m['T'], m['n']
    Z = _cplx(T)
    dq = np.concatenate([qd[None], np.eye(n, dtype=T)]).astype(Z) * Z(1j * step)
    mom, en = _momentum_energy(m, q[None].astype(Z) + dq, qd.astype(Z), base, hbase, flaws)
    return (mom[0].imag - en[1:].imag) / T(step)


def joint_dynamics(m, st, flaws=(), step=STEP):
    """dict(minv [ndof, ndof], qdd [ndof], M, h, dead: the DoFs that count as frozen, pos / rot: the link frames) of one state"""
    T, n = m['T'], m['n']
    q, qd = np.asarray(st['q'], dtype=T), np.asarray(st['qd'], dtype=T)
    P, R = fk(m, q[None], st['base'], st['hbase'])
    Jv, Jw, Iw, cw = jacobians(m, P, R)
    if any(f.startswith('com_inertia') for f in flaws):
        M = mass_matrix(m, *jacobians(m, P, R, _com_scale(m, flaws))[:3])[0]
    else:
        M = mass_matrix(m, Jv, Jw, Iw)[0]
    Jv, Jw, Iw = Jv[0], Jw[0], Iw[0]
    v, w = np.einsum('dki,k->di', Jv, qd), np.einsum('dki,k->di', Jw, qd)
    g = np.where(m['human'] & ('human_gravity' not in flaws), m['HUMAN_GRAVITY_Z'], m['ROBOT_GRAVITY_Z']).astype(T)
    quad = T(0 if 'linear_damping' in flaws else 1)
    sl = m['LIN_DAMP'] + quad * m['LIN_DAMP'] * np.sqrt((v * v).sum(1))
    sa = m['ANG_DAMP'] + quad * m['ANG_DAMP'] * np.sqrt((w * w).sum(1))
    F = -(m['mass'] * sl)[:, None] * v
    F[:, 2] += m['mass'] * g
    tau = -sa[:, None] * np.einsum('dij,dj->di', Iw, w)
    Qf = np.einsum('dki,di->k', Jv, F) + np.einsum('dki,di->k', Jw, tau) - _flag_scale(m, flaws, 'jdamp') * m['jdamp'] * qd
    C = velocity_products(m, q, qd, st['base'], st['hbase'], step, flaws) if 'no_velocity_products' not in flaws else np.zeros(n, dtype=T)
    h = C - Qf
    frozen = 0 if 'frozen_live' in flaws else int(st['frozen'])
    dead = np.array([(d < 32 and (frozen >> d) & 1 == 1) or not M[d, d] > DEAD_ROW for d in range(n)])
    minv, qdd = np.zeros((n, n), dtype=T), np.zeros(n, dtype=T)
    for b0, b1 in ((0, m['nrobot']), (m['nrobot'], n)):
        live = np.nonzero(~dead[b0:b1])[0] + b0
        if len(live):
            inv = np.linalg.inv(M[np.ix_(live, live)])
            minv[np.ix_(live, live)] = inv
            qdd[live] = inv @ -h[live]
    assert minv.dtype == T and qdd.dtype == T and h.dtype == T
    out = dict(minv=minv, qdd=qdd, M=M, h=h, dead=dead, pos=P[0], rot=R[0], C=C)
    if m.get('ee') is not None:
        out['e'], out['eq'] = point_terms(m, P[0], R[0], cw[0], Iw, minv, qdd, qd, v, w, g, sl, sa)
    return out


def point_terms(m, P, R, cw, Iw, minv, qdd, qd, v, w, grav, sl, sa):
    """(e, eq) of LIMITS, each [ndof]: what forming every link's inertia and bias force about the kernel's reference point r leaves of
    M^-1 -- entry (a, b) at most e_a e_b -- and of qdd.  P, R: link frames, cw: centres of mass, Iw: world inertias, v, w: the links'
    velocities at their centres of mass and angular velocities, grav, sl, sa: their gravity and damping factors"""
    eps = np.sqrt(POINT_ROUNDINGS / 3) * 2.0 ** -24      # a rounding error is uniform over half an ulp either way: variance (half an ulp)^2 / 3
    r = P[m['ee']]
    aw = np.einsum('dij,dj->di', R, m['axis'])
    c = cw - r
    wk = m['rev']                                                                          # |angular part| of joint k's unit twist: 1 revolute, 0 prismatic
    vk = np.where(m['rev'] > 0, np.sqrt((_cross(aw, r - P) ** 2).sum(1)), 1.0)             # |linear part at r|
    g = np.sqrt((_cross(aw[None, :, :], c[:, None, :]) ** 2).sum(2)) * wk[None, :] + vk[None, :]      # g[l, k] = |w_k x (c_l - r)| + |v_k|
    In = np.array([np.linalg.norm(I, 2) for I in Iw])
    aw_, ag_ = m['anc'] * wk[None, :], m['anc'] * g
    T = np.einsum('lk,lj,l->lkj', aw_, aw_, In) + np.einsum('lk,lj,l->lkj', ag_, ag_, m['mass'])      # link l's terms in entry (k, j) of M
    V = eps ** 2 * (T ** 2).sum(0)                                                          # variance of dM, the links' roundings independent
    A2 = minv ** 2
    e = np.sqrt(SIGMAS * np.sqrt(np.maximum(np.einsum('ak,kj,aj->a', A2, V, A2), 0.0)))
    # the bias force of link l about r: w x (I w + c x m v_c) + v_o x m v_c, w x m v_c, less the external (tau + c x f, f), term by term
    nw, nc = np.sqrt((w * w).sum(1)), np.sqrt((c * c).sum(1))
    nvo = np.sqrt(((v - _cross(w, c)) ** 2).sum(1))                                        # the link's velocity at r
    sp = nvo + nw * nc                                                                     # the pieces of v_c = v_o + w x c
    f = m['mass'] * (np.abs(grav) + sl * sp)
    ang = nw * (In * nw + m['mass'] * nc * sp) + nvo * m['mass'] * sp + sa * In * nw + nc * f
    lin = nw * m['mass'] * sp + f
    par = m['parent']
    wpar = np.array([nw[par[d]] if par[d] >= 0 else 0.0 for d in range(m['n'])])           # the velocity-product acceleration of joint d: |w_parent| |qd_d| x its twist
    Vh = eps ** 2 * ((m['anc'] ** 2).T @ ang ** 2 * wk ** 2 + (m['anc'] ** 2).T @ lin ** 2 * vk ** 2) + V @ (wpar * qd) ** 2
    return e, SIGMAS * np.sqrt(A2 @ (V @ qdd ** 2 + Vh))


def free_dynamics(m, st, flaws=()):
    """the free bodies' records [nfree, 13] after one substep"""
    T = m['T']
    fr = np.array(st['free'], dtype=T).reshape(-1, 13)
    out = fr.copy()
    dt, kl, ka = m['DT'], m['LIN_DAMP'], m['ANG_DAMP']
    for b, r in enumerate(fr):
        x, R, v, w = r[:3], quat_mat(r[3:7], T), r[7:10], r[10:13]
        I = m['freeb'][b, FB['inertia']:FB['inertia'] + 3]
        Ii = np.array([1 / i if i > 0 else 0 for i in I], dtype=T)
        v2 = v + dt * (np.array([0, 0, m['freeb'][b, FB['gravity']]], dtype=T) - (kl + kl * np.sqrt(v @ v)) * v)
        Lw = R @ (I * (R.T @ w))
        acc = R @ (Ii * (R.T @ -_cross(w, Lw)))
        w2 = w + dt * (acc - (ka + ka * np.sqrt(w @ w)) * w)
        wn = np.sqrt(w2 @ w2)
        th = wn * dt
        if th > SMALL_ANGLE and 'small_angle' not in flaws:
            dq = np.concatenate([w2 * (np.sin(th / 2) / wn), [np.cos(th / 2)]]).astype(T)
        else:
            dq = np.concatenate([w2 * (dt / 2), [1]]).astype(T)
        a, c = dq, r[3:7]      # the Hamilton product dq q, (x, y, z, w)
        qn = np.array([a[3] * c[0] + a[0] * c[3] + a[1] * c[2] - a[2] * c[1], a[3] * c[1] - a[0] * c[2] + a[1] * c[3] + a[2] * c[0],
                       a[3] * c[2] + a[0] * c[1] - a[1] * c[0] + a[2] * c[3], a[3] * c[3] - a[0] * c[0] - a[1] * c[1] - a[2] * c[2]], dtype=T)
        out[b, :3], out[b, 3:7], out[b, 7:10], out[b, 10:13] = x + dt * v2, qn / np.sqrt(qn @ qn), v2, w2
    assert out.dtype == T
    return out


def reference(links, freeb, par, nrobot, st, T=np.float64, flaws=(), step=STEP, ee=None):
    """one substep of one environment.  links [2, ndof, LINK_COLS]; st: dict(q, qd, base, hbase, free, gender, frozen)"""
    lk = np.asarray(links)
    g = 0 if 'gender0' in flaws else int(st['gender'])
    rows = np.concatenate([lk[0, :nrobot], lk[g, nrobot:]])
    m = model_of(rows, freeb, par, nrobot, T)
    m['ee'] = ee      # the link whose origin the kernel's spatial algebra is referred to (AGX_T_EE_LINK): with it the result carries E
    out = joint_dynamics(m, st, flaws, step)
    out['free'] = free_dynamics(m, st, flaws) if freeb is not None and len(freeb) else np.zeros((0, 13), dtype=T)
    return out


def iterate(links, freeb, par, nrobot, st, steps, T=np.float64, ee=None):
    """`steps` substeps of the reference from state st: qd' = qd + dt qdd, q' = q + dt qd', the free bodies by their own rule.  Returns
    dict(q, qd, free; with `ee`: eq_q, eq_qd, what the raised term eq of every substep adds up to in q and qd)"""
    dt = T(par['DT'])
    s = dict(st, q=np.asarray(st['q'], dtype=T), qd=np.asarray(st['qd'], dtype=T))
    n = len(s['q'])
    eq_q, eq_qd = np.zeros(n), np.zeros(n)
    for _ in range(steps):
        r = reference(links, freeb, par, nrobot, s, T, ee=ee)
        qd = s['qd'] + dt * r['qdd']
        s = dict(s, q=s['q'] + dt * qd, qd=qd, free=r['free'])
        if ee is not None:
            eq_qd = eq_qd + float(dt) * r['eq']
            eq_q = eq_q + float(dt) * eq_qd
    assert s['q'].dtype == T and s['qd'].dtype == T
    return dict(q=s['q'], qd=s['qd'], free=s['free'], eq_q=eq_q, eq_qd=eq_qd)


def measures_iterated(links, freeb, par, nrobot, st, ref, steps, seed):
    """(S, D32), each [2]: of q and of qd after `steps` substeps, as measures() takes them of one"""
    rng = np.random.RandomState(seed)
    lk = np.asarray(links, dtype=np.float32)
    dev = lambda a: np.array([np.abs(np.asarray(a['q'], dtype=np.float64) - ref['q']).max(), np.abs(np.asarray(a['qd'], dtype=np.float64) - ref['qd']).max()])
    S = np.zeros(2)
    for _ in range(SENS_TRIALS):
        l2 = lk.copy()
        l2[:, :, LK['tpos']:] = _nudge(lk[:, :, LK['tpos']:], rng)
        f2 = None if freeb is None else _nudge(freeb, rng)
        p2 = {k: _nudge(np.float32(v), rng) for k, v in par.items()}
        s2 = dict(st, **{k: _nudge(st[k], rng) for k in ('q', 'qd', 'base', 'hbase', 'free')})
        S = np.maximum(S, dev(iterate(l2, f2, p2, nrobot, s2, steps)))
    return S, dev(iterate(lk, None if freeb is None else np.asarray(freeb, dtype=np.float32), par, nrobot, st, steps, np.float32))


# ---------------------------------------------------------------------------------------------------- limits
def ulp32(a):
    return float(np.spacing(np.float32(np.abs(a).max()))) if np.size(a) else 0.0


def _nudge(a, rng):
    a = np.asarray(a, dtype=np.float32)
    b = np.where(rng.rand(*a.shape) < 0.5, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf)))
    return np.where(a == 0, a, b).astype(np.float32)      # an exact zero (a massless link, a body at rest, an absent term) is a statement, not a rounded number


def _blocks(n, nrobot):
    return ((0, nrobot), (nrobot, n))


def deviations(a, b, nrobot):
    """(the four joint quantities of QUANT, free bodies [nfree, 4]): largest differences of two results of reference()"""
    n = len(a['qdd'])
    j = [float(np.abs(a['minv'][b0:b1, b0:b1] - b['minv'][b0:b1, b0:b1]).max()) if b1 > b0 else 0.0 for b0, b1 in _blocks(n, nrobot)] + \
        [float(np.abs(a['qdd'][b0:b1] - b['qdd'][b0:b1]).max()) if b1 > b0 else 0.0 for b0, b1 in _blocks(n, nrobot)]
    d = np.abs(np.asarray(a['free'], dtype=np.float64) - np.asarray(b['free'], dtype=np.float64))
    sgn = np.abs(np.asarray(a['free'], dtype=np.float64)[:, 3:7] + np.asarray(b['free'], dtype=np.float64)[:, 3:7])      # q and -q are one rotation
    f = np.stack([d[:, :3].max(1), np.minimum(d[:, 3:7].max(1), sgn.max(1)), d[:, 7:10].max(1), d[:, 10:13].max(1)], 1) if len(d) else np.zeros((0, 4))
    return np.array(j), f


def scales(ref, nrobot):
    n = len(ref['qdd'])
    j = [float(np.abs(ref['minv'][b0:b1, b0:b1]).max()) if b1 > b0 else 0.0 for b0, b1 in _blocks(n, nrobot)] + \
        [float(np.abs(ref['qdd'][b0:b1]).max()) if b1 > b0 else 0.0 for b0, b1 in _blocks(n, nrobot)]
    fr = np.abs(np.asarray(ref['free'], dtype=np.float64))
    f = np.stack([fr[:, :3].max(1), np.ones(len(fr)), fr[:, 7:10].max(1), fr[:, 10:13].max(1)], 1) if len(fr) else np.zeros((0, 4))
    return np.array(j), f


def measures(links, freeb, par, nrobot, st, ref, seed):
    """(S, D32) of one environment, each (joint quantities [4], free bodies [nfree, 4])"""
    rng = np.random.RandomState(seed)
    Sj, Sf = np.zeros(4), np.zeros((len(ref['free']), 4))
    lk = np.asarray(links, dtype=np.float32)
    for _ in range(SENS_TRIALS):
        l2 = lk.copy()
        l2[:, :, LK['tpos']:] = _nudge(lk[:, :, LK['tpos']:], rng)
        f2 = None if freeb is None else _nudge(freeb, rng)
        p2 = {k: _nudge(np.float32(v), rng) for k, v in par.items()}
        s2 = dict(st, **{k: _nudge(st[k], rng) for k in ('q', 'qd', 'base', 'hbase', 'free')})
        j, f = deviations(reference(l2, f2, p2, nrobot, s2), ref, nrobot)
        Sj, Sf = np.maximum(Sj, j), np.maximum(Sf, f)
    r32 = reference(lk, None if freeb is None else np.asarray(freeb, dtype=np.float32), par, nrobot, st, np.float32)
    Dj, Df = deviations(r32, ref, nrobot)
    return (Sj, Sf), (Dj, Df)


def limits(S, D32, scale):
    """(limit, whether the pose may be stored): 4 max(S, D32), floored at FLOOR_ULPS ulp32 of the scale; not storable where that reaches CAP x scale"""
    S, D32, scale = (np.asarray(x, dtype=np.float64) for x in (S, D32, scale))
    raw = 4 * np.maximum(S, D32)
    floor = FLOOR_ULPS * np.spacing(scale.astype(np.float32)).astype(np.float64) * (scale > 0)
    return np.maximum(raw, floor), bool((raw < CAP * scale)[scale > 0].all())


# ---------------------------------------------------------------------------------------------------- the stored cases
_CACHE = {}


def load_cases(path=GOLDEN):
    if path not in _CACHE:
        z = np.load(path)
        _CACHE[path] = {k: (json.loads(str(z[k])) if k.endswith('/recipe') else z[k]) for k in z.files}
    return _CACHE[path]


def scenes(cases):
    return [k[:-len('/recipe')] for k in cases if k.endswith('/recipe')]


def scene_blob(cases, name):
    from assistive_gym_amd.blob import ModelBlob
    key = ('blob', name, id(cases))
    if key not in _CACHE:
        rec = cases[name + '/recipe']
        _CACHE[key] = splice(ModelBlob.load(rec['model']), cases[name + '/links'], cases[name + '/freeb'] if len(cases[name + '/freeb']) else None, rec['params'])
    return _CACHE[key]


def pose_of(cases, name, p):
    """dict(q, qd, base, hbase, free, gender, frozen) of stored pose p"""
    return dict(q=cases[name + '/q'][p], qd=cases[name + '/qd'][p], base=cases[name + '/base'][p], hbase=cases[name + '/hbase'][p], free=cases[name + '/free'][p],
                gender=int(cases[name + '/env'][p, 0]), frozen=int(cases[name + '/env'][p, 1]))


def make_state(blob, st):
    """a state record that holds the pose and nothing else: every body at the origin, upright and at rest, no food, no tremor"""
    s = blob.new_state(1)
    v = blob.view(s)
    v['q'][0], v['qd'][0], v['qt'][0] = st['q'], st['qd'], st['q']
    v['base'][0] = st['base']
    v['human'][0, :, 6] = 1.0
    v['human'][0, 0] = st['hbase']
    if blob.nfree:
        v['free'][0] = np.asarray(st['free']).reshape(blob.nfree, 13)
    v['gender'][0], v['frozen'][0], v['limit_scale'][0], v['plane_friction'][0] = st['gender'], st['frozen'], 1.0, 1.0
    return s[0]


def scene_states(cases, name):
    blob = scene_blob(cases, name)
    return np.stack([make_state(blob, pose_of(cases, name, p)) for p in range(len(cases[name + '/q']))])


def tri(n):
    return np.triu_indices(n)


def pack_vec(v):
    """numbers as the file holds them: float32, and what float32 leaves of them in steps of 1/254 of a float32 ulp of the largest (int8).  The
    stored value differs from the float64 one by at most half a step, a thousandth of the smallest limit"""
    v = np.asarray(v, dtype=np.float64)
    hi = v.astype(np.float32)
    step = float(np.spacing(np.abs(hi).max())) / 254 if v.size and np.abs(hi).max() > 0 else 1.0
    return hi, np.clip(np.rint((v - hi.astype(np.float64)) / step), -127, 127).astype(np.int8)


def unpack_vec(hi, lo):
    step = float(np.spacing(np.abs(hi).max())) / 254 if hi.size and np.abs(hi).max() > 0 else 1.0
    return hi.astype(np.float64) + lo.astype(np.float64) * step


def pack_sym(blk):
    """a symmetric block: its upper triangle, packed (pack_vec)"""
    return pack_vec(blk[tri(len(blk))])


def unpack_sym(hi, lo):
    n = int(round((np.sqrt(8 * len(hi) + 1) - 1) / 2))
    blk = np.zeros((n, n))
    blk[tri(n)] = unpack_vec(hi, lo)
    return blk + np.triu(blk, 1).T


def stored_qdd(cases, name, p):
    rec = cases[name + '/recipe']
    return np.concatenate([unpack_vec(cases[name + '/qdd_%s_hi' % k][p], cases[name + '/qdd_%s_lo' % k][p]) for k in 'rh'])[:rec['ndof']]


def stored_minv(cases, name, p):
    """the stored M^-1 of pose p: the upper triangles of the two blocks (pack_sym), unfolded"""
    rec = cases[name + '/recipe']
    n, nr = rec['ndof'], rec['nrobot']
    out = np.zeros((n, n))
    for key, (b0, b1) in zip(('minv_r', 'minv_h'), _blocks(n, nr)):
        if b1 > b0:
            out[b0:b1, b0:b1] = unpack_sym(cases[name + '/' + key + '_hi'][p], cases[name + '/' + key + '_lo'][p])
    return out


def stored_result(cases, name, p):
    return dict(minv=stored_minv(cases, name, p), qdd=stored_qdd(cases, name, p), free=unpack_vec(cases[name + '/free_next_hi'][p], cases[name + '/free_next_lo'][p]), dead=cases[name + '/dead'][p].astype(bool))


def expected_rows(blob):
    """the rows an isolated scene still builds: the six of every tool's fixed constraint, inert between limits of 0"""
    if not blob.nfree:
        return 0
    return 6 * (2 if blob.task_kind == L.TASK_ARM_MANIPULATION and blob.task_i('TOOL2_BODY') > 0 else 1)


# ---------------------------------------------------------------------------------------------------- judging a result
def result_of(dbg, lay, state_after, blob):
    """what judge looks at, from one environment's debug record (layout `lay`: agx_debug_layout) and its state record after the substep"""
    dbg = np.asarray(dbg, dtype=np.float32)
    n, stride = blob.ndof, lay[3]
    v = blob.view(np.asarray(state_after, dtype=np.float32).reshape(1, -1))
    return dict(ncon=int(dbg[0]), nrows=int(dbg[1]), minv=dbg[lay[2]:lay[2] + stride * stride].reshape(stride, stride)[:n, :n].copy(), qdd=dbg[lay[7]:lay[7] + n].copy(),
                q=v['q'][0].copy(), qd=v['qd'][0].copy(), free=v['free'][0].copy())


def perfect(cases, name, p, ref=None):
    """the record of a device that computes `ref` (the stored values if None) exactly, rounded to float32"""
    st = pose_of(cases, name, p)
    ref = ref or stored_result(cases, name, p)
    dt = float(np.float32(cases[name + '/recipe']['dt']))
    qdd = np.asarray(ref['qdd'], dtype=np.float32)
    qd = (np.asarray(st['qd'], dtype=np.float64) + dt * qdd.astype(np.float64)).astype(np.float32)
    q = (np.asarray(st['q'], dtype=np.float64) + dt * qd.astype(np.float64)).astype(np.float32)
    blob = scene_blob(cases, name)
    return dict(ncon=0, nrows=expected_rows(blob), minv=np.asarray(ref['minv'], dtype=np.float32), qdd=qdd, q=q, qd=qd, free=np.asarray(ref['free'], dtype=np.float32))


def _half_ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64) / 2


def _is_update(got, a, dt, b):
    """float32 `got` is a + dt b (float64) as float32 arithmetic can leave it: half an ulp of the sum, and -- unless the compiler contracts
    the update -- half an ulp of the product before it; one ulp of the sum in all where nothing cancels"""
    want = a + dt * b
    return np.abs(got.astype(np.float64) - want) <= _half_ulp(want) + _half_ulp(dt * b)


def compare(res, want, lim, e, eq, flim, st, dt, nrobot, rows, loose=False):
    """One environment: a result (result_of) against the stored one.  Returns (maxima as fractions of the limits and absolute, violations)"""
    n = len(want['qdd'])
    bad = []
    m = dict(minv=0.0, minv_of=0.0, sym_of=0.0, qdd=0.0, qdd_of=0.0, free_of=0.0, quat_norm=0.0)
    if res['ncon'] != 0 or res['nrows'] != rows:
        bad.append('%d contacts and %d rows, want 0 and %d: the scene is not isolated' % (res['ncon'], res['nrows'], rows))
    G, q = res['minv'], res['qdd']
    if not (np.isfinite(G).all() and np.isfinite(q).all() and np.isfinite(res['free']).all() and np.isfinite(res['q']).all() and np.isfinite(res['qd']).all()):
        return m, bad + ['not finite']
    for b, (b0, b1) in enumerate(_blocks(n, nrobot)):
        if b1 == b0:
            continue
        em = np.abs(G[b0:b1, b0:b1].astype(np.float64) - want['minv'][b0:b1, b0:b1])
        s = np.abs(G[b0:b1, b0:b1].astype(np.float64) - G[b0:b1, b0:b1].astype(np.float64).T)
        eqd = np.abs(q[b0:b1].astype(np.float64) - want['qdd'][b0:b1])
        who = 'robot' if b == 0 else 'human'
        sm, sq = np.abs(want['minv'][b0:b1, b0:b1]).max(), np.abs(want['qdd'][b0:b1]).max()
        lm, lq = np.minimum(lim[b] + np.outer(e[b0:b1], e[b0:b1]), max(CAP * sm, lim[b])), np.minimum(lim[2 + b] + eq[b0:b1], max(CAP * sq, lim[2 + b]))
        if loose:      # the bound the suite held before these cases: CAP of the block's largest entry, whatever the entry
            lm, lq = CAP * sm + 0 * lm, CAP * sq + 0 * lq
        for what, err, l, key in (('M^-1', em, lm, 'minv'), ('M^-1 - M^-T', s, lm, 'sym'), ('qdd', eqd, lq, 'qdd')):
            if key != 'sym':
                m[key] = max(m[key], float(err.max()))
            with np.errstate(divide='ignore', invalid='ignore'):
                frac = np.where(l > 0, err / np.where(l > 0, l, 1), np.where(err == 0, 0.0, np.inf))
            m[key + '_of'] = max(m[key + '_of'], float(frac.max()))
            if not (err <= l).all():
                at = np.unravel_index(int(np.argmax(frac)), err.shape)
                bad.append('%s of the %s block off by %.3g at %s, limit %.3g' % (what, who, err[at], tuple(int(x) + b0 for x in at), l[at]))
    cross = np.concatenate([G[:nrobot, nrobot:].reshape(-1), G[nrobot:, :nrobot].reshape(-1)])
    if (cross != 0).any():
        bad.append('M^-1 has %d non-zero entries across the blocks, the largest %.3g' % ((cross != 0).sum(), np.abs(cross).max()))
    dead = want['dead']
    if (G[dead, :] != 0).any() or (G[:, dead] != 0).any() or (q[dead] != 0).any():
        bad.append('a frozen DoF has a non-zero row or column of M^-1 or a non-zero qdd')
    # the stored state: the update from the device's own qdd, then from its own qd'
    if not _is_update(res['qd'], np.asarray(st['qd'], dtype=np.float32).astype(np.float64), dt, q.astype(np.float64)).all():
        bad.append('qd\' is not qd + dt qdd: ')
    if not _is_update(res['q'], np.asarray(st['q'], dtype=np.float32).astype(np.float64), dt, res['qd'].astype(np.float64)).all():
        bad.append('q\' is not q + dt qd\': ')
    if len(want['free']):
        f, w = res['free'].astype(np.float64), np.asarray(want['free'], dtype=np.float64)
        d = np.abs(f - w)
        dq = np.minimum(d[:, 3:7].max(1), np.abs(f[:, 3:7] + w[:, 3:7]).max(1))
        err = np.stack([d[:, :3].max(1), dq, d[:, 7:10].max(1), d[:, 10:13].max(1)], 1)
        with np.errstate(divide='ignore', invalid='ignore'):
            frac = np.where(flim > 0, err / np.where(flim > 0, flim, 1), np.where(err == 0, 0.0, np.inf))
        m['free_of'] = float(frac.max())
        for b, k in zip(*np.nonzero(~(err <= flim))):
            bad.append('free body %d: %s off by %.3g, limit %.3g' % (b, ('position', 'quaternion', 'v', 'w')[k], err[b, k], flim[b, k]))
        nq = np.abs(np.sqrt((f[:, 3:7] ** 2).sum(1)) - 1)
        m['quat_norm'] = float(nq.max() / np.spacing(np.float32(1)))
        if not (nq <= 2 * np.spacing(np.float32(1))).all():
            bad.append('a free body\'s quaternion has norm 1 %+.3g' % nq.max())
    return m, bad


def qdd_limits(cases, name, p):
    """(limit of qdd per DoF as compare applies it, the blocks' scales per DoF) of stored pose p"""
    rec = cases[name + '/recipe']
    want, lim, eq = stored_qdd(cases, name, p), cases[name + '/lim'][p], cases[name + '/eq'][p]
    out, scale = np.zeros(rec['ndof']), np.zeros(rec['ndof'])
    for b, (b0, b1) in enumerate(_blocks(rec['ndof'], rec['nrobot'])):
        if b1 > b0:
            scale[b0:b1] = np.abs(want[b0:b1]).max()
            out[b0:b1] = np.minimum(lim[2 + b] + eq[b0:b1], max(CAP * scale[b0], lim[2 + b]))
    return out, scale


def judge(cases, name, results, only=None, loose=False):
    """results: per stored pose a dict of result_of / perfect.  Returns (maxima over the scene, violations).  only: the poses to look at (all
    of them if None); loose: judge M^-1 and qdd by CAP x scale alone, as the suite did before (tests/test_dynamics_cases.py shows what that lets pass)"""
    rec = cases[name + '/recipe']
    npose = len(cases[name + '/q'])
    assert len(results) == npose
    rows = expected_rows(scene_blob(cases, name))
    tot = dict(n=0, minv=0.0, minv_of=0.0, sym_of=0.0, qdd=0.0, qdd_of=0.0, free_of=0.0, quat_norm=0.0, lim_minv=float(cases[name + '/lim'][:, :2].max() + cases[name + '/e'].max() ** 2), lim_qdd=float(cases[name + '/lim'][:, 2:].max()))
    bad = []
    for p, res in enumerate(results):
        if only is not None and p not in only:
            continue
        m, b = compare(res, stored_result(cases, name, p), cases[name + '/lim'][p], cases[name + '/e'][p], cases[name + '/eq'][p], cases[name + '/flim'][p], pose_of(cases, name, p), float(np.float32(rec['dt'])), rec['nrobot'], rows, loose)
        bad += ['pose %d: %s' % (p, t) for t in b]
        for k in m:
            tot[k] = max(tot[k], m[k])
        tot['n'] += 1
    return tot, bad


def judge_iterated(cases, name, results):
    """results: per stored pose (q, qd) after the scene's `steps` substeps.  Returns (maxima, violations): q and qd of every DoF against the
    reference iterated as often, limits 4 max(S, D32) of the iteration + what eq adds up to, the cap as in compare"""
    tot, bad = dict(n=0, q=0.0, q_of=0.0, qd=0.0, qd_of=0.0), []
    for p, (q, qd) in enumerate(results):
        for k, (got, key) in enumerate(((q, 'q'), (qd, 'qd'))):
            want, base = unpack_vec(cases[name + '/' + key + '4_hi'][p], cases[name + '/' + key + '4_lo'][p]), cases[name + '/lim4'][p, k]
            lim = np.minimum(base + cases[name + '/e4'][p, k], max(CAP * np.abs(want).max(), base))
            err = np.abs(np.asarray(got, dtype=np.float64) - want)
            tot[key], tot[key + '_of'] = max(tot[key], float(err.max())), max(tot[key + '_of'], float((err / lim).max()))
            if not (np.isfinite(err).all() and (err <= lim).all()):
                a = int(np.argmax(err / lim))
                bad.append('pose %d: %s of DoF %d off by %.3g after the substeps, limit %.3g' % (p, key, a, err[a], lim[a]))
        tot['n'] += 1
    return tot, bad


# ---------------------------------------------------------------------------------------------------- the other two kinematics walks
def mat_quat(R):
    """quaternion (x, y, z, w) of a rotation matrix"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax([R[0, 0], R[1, 1], R[2, 2], t]))
    if k == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1 + t])
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q = np.zeros(4)
        q[i], q[j], q[l], q[3] = 1 + R[i, i] - R[j, j] - R[l, l], R[i, j] + R[j, i], R[i, l] + R[l, i], R[l, j] - R[j, l]
    return q / np.sqrt(q @ q)


def frames(links, par, nrobot, st, ee, ee_pos, ee_quat, T=np.float64):
    """(positions [nrobot + 1, 3], rotations [nrobot + 1, 3, 3]) of the robot's link frames and, last, of the end-effector frame: the frame
    (ee_pos, ee_quat) in the frame of link `ee` (AGX_T_EE_LINK, AGX_T_EE_POS, AGX_T_EE_QUAT)"""
    lk = np.asarray(links)
    m = model_of(np.concatenate([lk[0, :nrobot], lk[int(st['gender']), nrobot:]]), None, par, nrobot, T)
    P, R = fk(m, np.asarray(st['q'], dtype=T)[None], st['base'], st['hbase'])
    P, R = P[0], R[0]
    pe, Re = R[ee] @ np.asarray(ee_pos, dtype=T) + P[ee], R[ee] @ quat_mat(ee_quat, T)
    out = np.concatenate([P[:nrobot], pe[None]]), np.concatenate([R[:nrobot], Re[None]])
    assert out[0].dtype == T and out[1].dtype == T
    return out


def frame_limits(links, par, nrobot, st, ee, ee_pos, ee_quat, ref, seed):
    """[2]: the limits of a frame's position and of the entries of its rotation: 4 max(S, D32) of the frames, floored at FLOOR_ULPS ulp32 of the
    largest coordinate (of 1), S and D32 as measures() takes them"""
    rng = np.random.RandomState(seed)
    lk = np.asarray(links, dtype=np.float32)
    dev = lambda f: np.array([np.abs(f[0].astype(np.float64) - ref[0]).max(), np.abs(f[1].astype(np.float64) - ref[1]).max()])
    S = np.zeros(2)
    for _ in range(SENS_TRIALS):
        l2 = lk.copy()
        l2[:, :, LK['tpos']:] = _nudge(lk[:, :, LK['tpos']:], rng)
        s2 = dict(st, **{k: _nudge(st[k], rng) for k in ('q', 'base', 'hbase')})
        S = np.maximum(S, dev(frames(l2, par, nrobot, s2, ee, _nudge(ee_pos, rng), _nudge(ee_quat, rng))))
    D = dev(frames(lk, par, nrobot, st, ee, ee_pos, ee_quat, np.float32))
    return limits(S, D, np.array([np.abs(ref[0]).max(), 1.0]))[0]


def blob_ee(blob):
    return blob.task_i('EE_LINK'), blob.task_f('EE_POS', 3).astype(np.float32), blob.task_f('EE_QUAT', 4).astype(np.float32)


def judge_frames(cases, name, blob, collider_frames=None, ee_pose=None):
    """collider_frames: float32 [poses, ncoll, 12] (agx_collider_frames), ee_pose: float32 [poses, 7] (agx_ee_pose), either may be None.
    Against the stored frames: every collider on a robot link, and the end-effector frame.  Returns (maxima, violations, colliders compared)"""
    tot, bad, ncmp = dict(pos=0.0, pos_of=0.0, rot=0.0, rot_of=0.0), [], 0
    cols = [(c, blob.collider(c)['body']) for c in range(blob.h['NCOLL'])]
    cols = [(c, b) for c, b in cols if 0 <= b < blob.nrobot]
    for p in range(len(cases[name + '/q'])):
        pos = unpack_vec(cases[name + '/fpos_hi'][p], cases[name + '/fpos_lo'][p])
        rot = np.stack([quat_mat(q) for q in unpack_vec(cases[name + '/fquat_hi'][p], cases[name + '/fquat_lo'][p])])
        lp, lr = cases[name + '/frame_lim'][p]
        got = []
        if collider_frames is not None:
            got += [('collider %d' % c, collider_frames[p, c, :3], collider_frames[p, c, 3:].reshape(3, 3), b) for c, b in cols]
            ncmp += len(cols)
        if ee_pose is not None:
            got.append(('end effector', ee_pose[p, :3], quat_mat(ee_pose[p, 3:7]), len(pos) - 1))
        for what, gp, gr, k in got:
            ep, er = np.abs(gp.astype(np.float64) - pos[k]).max(), np.abs(np.asarray(gr, dtype=np.float64) - rot[k]).max()
            tot['pos'], tot['pos_of'], tot['rot'], tot['rot_of'] = max(tot['pos'], ep), max(tot['pos_of'], ep / lp), max(tot['rot'], er), max(tot['rot_of'], er / lr)
            if not (ep <= lp and er <= lr):
                bad.append('pose %d, %s: position off by %.3g (limit %.3g), rotation by %.3g (limit %.3g)' % (p, what, ep, lp, er, lr))
    return tot, bad, ncmp


def say(name, who, m):
    return ('dynamics %-10s %-8s poses %3d | M^-1 %.3g, %.2f of its limit at most (limits <= %.3g), asymmetry %.2f | qdd %.3g, %.2f of its limit (<= %.3g) | free bodies %.2f of their limits, | |quat| - 1 | %.1f ulp'
            % (name, who, m['n'], m['minv'], m['minv_of'], m['lim_minv'], m['sym_of'], m['qdd'], m['qdd_of'], m['lim_qdd'], m['free_of'], m['quat_norm']))
