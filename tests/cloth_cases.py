"""Small synthetic garments for the cloth kernel (csrc/agx_cloth.h) and the oracle's cloth_substep: a grid of nodes spliced into the
DressingBaxter blob in place of the hospital gown, a deliberately plain numpy restatement of one internal substep (written independently
of the C code and of the kernel: what the sides share is the blob), and the comparison the device tests judge by.

  grid_obj / splice / tables        the garment: grid size and spacing, anchors, shape list, parameter overrides
  numpy_substep                     the first restatement: one capsule, float64 (tests/test_cloth_oracle.py)
  substep                           everything the kernel does per substep: a list of shapes in blob shape order (capsule / sphere cores
                                    exactly, hulls through the blob's own plane table), the shapes' gender filter, the two-contact cap,
                                    anchored nodes that never collide, float32 or float64 arithmetic, and the margin of every branch
  determined                        is every branch of a substep clear of its threshold?
  compare                           device (or planted) output against the stored float64 result, all nodes, maxima

A plain module, not a conftest.  tests/diag/make_cloth_kernel_cases.py writes tests/golden/cloth_kernel_cases.npz with it."""
import os
import tempfile

import numpy as np

from assistive_gym_amd.model import compiler as L

EPS = 1.1920929e-7          # SIMD_EPSILON
NODE_CONTACTS = L.CLOTH_NODE_CONTACTS
PARAMS = dict(KLST=0.055, KDP=0.01, KDG=10.0, KDF=0.39, KCHR=1.0, KKHR=1.0, KAHR=1.0, PITER=5, MARGIN=0.04, AIR_DENSITY=1.2, FORCE_SCALE=10.0, FORCE_MAX=20.0, EE_BELOW=0.05)
# bands of a determined substep (every node, every iteration)
BAND = dict(dst=1e-5, dn=2e-6, friction=1e-3, clamp=1e-3, vn=1e-4, plane=1e-5)


def _grid_obj(path, nx=6, ny=5, h=0.03):
    with open(path, 'w') as f:
        for j in range(ny):
            for i in range(nx):
                f.write('v %f %f %f\n' % (i * h, j * h, 0.002 * ((i * 7 + j * 3) % 5)))      # slightly crumpled: normals are not all alike
        for j in range(ny - 1):
            for i in range(nx - 1):
                a, b, c, d = j * nx + i + 1, j * nx + i + 2, (j + 1) * nx + i + 2, (j + 1) * nx + i + 1
                f.write('f %d//%d %d//%d %d//%d\n' % (a, a, b, b, c, c))
                f.write('f %d//%d %d//%d %d//%d\n' % (a, a, c, c, d, d))


def gender_of(dr):
    r = dr.meta['ranges']
    return lambda ci: 1 if r['human_male'][0] <= ci < r['human_male'][1] else (2 if r['human_female'][0] <= ci < r['human_female'][1] else 0)


def forearm_capsule(dr, gender='male'):
    """collider index of the human's left forearm capsule: a two-vertex core on the link of human.left_elbow"""
    cands = [c for c in range(*dr.meta['ranges']['human_' + gender]) if len(dr.collider(c)['verts']) == 2 and dr.collider(c)['link'] == 17]
    assert cands, 'forearm capsule not found'
    return cands[0]


def splice(dr, nx=6, ny=5, h=0.03, anchors=(0, 5), shape_ids=(), overrides=None):
    """the DressingBaxter blob `dr` with an nx x ny grid garment of spacing h in place of the gown; node mass as the gown's.
    anchors: node indices, or 'centre': the two nodes nearest the middle of the patch"""
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.model.cloth import compile_cloth, load_obj_first_appearance
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, 'grid.obj')
        _grid_obj(obj, nx, ny, h)
        if isinstance(anchors, str):
            assert anchors == 'centre'
            V, _ = load_obj_first_appearance(obj)
            anchors = [int(k) for k in np.argsort(np.linalg.norm(V[:, :2] - V[:, :2].mean(0), axis=1), kind='stable')[:2]]
        colliders = [dr.collider(c) for c in range(dr.h['NCOLL'])]
        par = dict(PARAMS, MASS=0.16 * (nx * ny) / 3966)
        par.update(overrides or {})
        sec, meta = compile_cloth(obj, 1.0, [0, 0, 0], [0, 0, 0], list(anchors), [0.0, 0.0, 0.0], [0, 1, 2], [3, 4, 5], par, colliders, list(shape_ids), gender_of=gender_of(dr))
    oc = dr.h['OFF_CLOTH']
    w = np.concatenate([dr.words[:oc], sec])
    w[L.H['NWORDS']] = len(w)
    blob = ModelBlob(w, dr.meta)
    blob.cloth_meta = meta
    return blob


def one_substep_blob(blob):
    """SIM_SUBSTEPS = 1 and DT / 8: one settle(1) is exactly one internal substep (of the rigid scene and of the garment)"""
    from assistive_gym_amd.blob import ModelBlob
    w = blob.words.copy()
    w[L.H['SIM_SUBSTEPS']] = 1
    w.view(np.float32)[blob.h['OFF_PARAMS'] + L.P['DT']] = np.float32(0.02) / np.float32(8)
    return ModelBlob(w, blob.meta)


def tables(blob):
    oc = blob.h['OFF_CLOTH']
    ci, cf = blob.i[oc:], blob.f[oc:]
    nn, nl, ncol = int(ci[L.CL['NN']]), int(ci[L.CL['NL']]), int(ci[L.CL['NCOLOR']])
    lk = ci[ci[L.CL['OFF_LINK']]:ci[L.CL['OFF_LINK']] + 2 * nl].reshape(nl, 2)[:, 0]
    node = ci[ci[L.CL['OFF_NODE']]:ci[L.CL['OFF_NODE']] + 2 * (nn + 1)].reshape(nn + 1, 2)[:, 0]
    area = cf[ci[L.CL['OFF_NODE']]:ci[L.CL['OFF_NODE']] + 2 * (nn + 1)].reshape(nn + 1, 2)[:nn, 1].astype(np.float64)
    nface = int(node[nn])
    face = ci[ci[L.CL['OFF_FACE']]:ci[L.CL['OFF_FACE']] + nface]
    anc = ci[ci[L.CL['OFF_ANCHOR']]:ci[L.CL['OFF_ANCHOR']] + 4 * int(ci[L.CL['NANCHOR']])].reshape(-1, 4)
    ancf = cf[ci[L.CL['OFF_ANCHOR']]:ci[L.CL['OFF_ANCHOR']] + 4 * int(ci[L.CL['NANCHOR']])].reshape(-1, 4)[:, 1:].astype(np.float64)
    par = cf[ci[L.CL['OFF_PARAM']]:ci[L.CL['OFF_PARAM']] + L.CP['COUNT']].astype(np.float64)
    real = lk >= 0                                   # -1: an empty slot of the kernel's bank schedule
    rest2 = cf[ci[L.CL['OFF_LINK']]:ci[L.CL['OFF_LINK']] + 2 * nl].reshape(nl, 2)[:, 1].astype(np.float64)
    color = ci[ci[L.CL['OFF_COLOR']]:ci[L.CL['OFF_COLOR']] + ncol + 1]
    cls = (np.searchsorted(color, np.arange(nl), side='right') - 1)[real]      # colour class of every real link, in blob order
    npatch = (L.CLOTH_THREADS // 64) * int(ci[L.CL['NPATCH_COLOR']])           # classes below this one stay inside one wave's patch
    return dict(nn=nn, a=(lk & 0xffff)[real], b=((lk >> 16) & 0xffff)[real], rest2=rest2[real], cls=cls, ncolor=ncol, first_cross=npatch,
                node=node, face=face, area=area, anchors=anc[:, 0], anchor_off=ancf, par=par,
                x0=cf[ci[L.CL['OFF_X0']]:ci[L.CL['OFF_X0']] + 3 * nn].reshape(nn, 3).astype(np.float64))


def numpy_substep(t, x, v, grav, dt, anchor, capsule=None, friction=0.5):
    """one internal substep, written independently of the C code; capsule = (p0, p1, radius) in world coordinates or None"""
    P = t['par']
    kLST, kDP, kDG, kDF, kAHR, mrg, im, rho = (P[L.CP[k]] for k in ('KLST', 'KDP', 'KDG', 'KDF', 'KAHR', 'MARGIN', 'NODE_IM', 'AIR_DENSITY'))
    nn = t['nn']
    x, v = x.copy(), v.copy()
    # normals from the incident faces (area weighted), then gravity and the one-sided drag
    for i in range(nn):
        n = np.zeros(3)
        for e in range(t['node'][i], t['node'][i + 1]):
            j, k = t['face'][e] & 0xffff, (t['face'][e] >> 16) & 0xffff
            n += np.cross(x[j] - x[i], x[k] - x[i])
        ln = np.linalg.norm(n)
        if ln > 1.1920929e-7:
            n /= ln
        v[i, 2] += grav * dt
        s2 = v[i] @ v[i]
        if s2 > 1.1920929e-7 and v[i] @ n > 0:
            f = t['area'][i] * (v[i] @ n) * s2 / 2 * rho * kDG            # magnitude of the drag, against the velocity
            if (f * dt * im) ** 2 > s2:
                v[i] = 0
            else:
                v[i] = v[i] - v[i] / np.sqrt(s2) * f * dt * im
    q = x.copy()
    x = q + v * dt
    contacts = {}
    if capsule is not None:
        p0, p1, rad = capsule
        for i in range(nn):
            if i in t['anchors']:
                continue
            u = np.clip((x[i] - p0) @ (p1 - p0) / ((p1 - p0) @ (p1 - p0)), 0, 1)
            d = x[i] - (p0 + u * (p1 - p0))
            dist = np.linalg.norm(d) - rad - mrg
            if dist < 0:
                n = d / np.linalg.norm(d)
                vr = x[i] - q[i]
                dn = vr @ n
                fv = vr - n * dn
                fc = kDF * friction
                contacts[i] = dict(n=n, off=-(n @ x[i]) + dist, c3=0.0 if fv @ fv < (dn * fc) ** 2 else 1 - fc, imp=np.zeros(3))
    for it in range(int(P[L.CP['PITER']])):
        for a, i in enumerate(t['anchors']):
            x[i] = x[i] - (x[i] - q[i]) + (anchor + t['anchor_off'][a] - x[i]) * kAHR
        for i, c in contacts.items():
            vr = x[i] - q[i]
            dn = vr @ c['n']
            if dn <= 1.1920929e-7:
                dp = min(x[i] @ c['n'] + c['off'], mrg)
                corr = vr - (vr - c['n'] * dn) * c['c3'] + c['n'] * dp
                x[i] = x[i] - corr
                c['imp'] += corr / (dt * im)
        for l in range(len(t['a'])):          # the blob lists the links class by class; within a class the order is immaterial
            a, b = t['a'][l], t['b'][l]
            d = x[b] - x[a]
            ln = d @ d
            if t['rest2'][l] + ln > 1.1920929e-7:
                k = (t['rest2'][l] - ln) / (t['rest2'][l] + ln) * kLST * 0.5
                x[a] -= d * k
                x[b] += d * k
    v = (x - q) / dt * (1 - kDP)
    return x, v, {i: (x[i].copy(), c['imp'] / dt) for i, c in contacts.items()}


# ---------------------------------------------------------------------------------------------------- the general restatement
def shape_table(blob):
    """the shapes of the cloth section in blob shape order: what the section and the collider records say about each"""
    oc = blob.h['OFF_CLOTH']
    ci, cf = blob.i[oc:], blob.f[oc:]
    ns = int(ci[L.CL['NSHAPE']])
    rec = ci[ci[L.CL['OFF_SHAPE']]:ci[L.CL['OFF_SHAPE']] + 4 * ns].reshape(ns, 4)
    out = []
    for c, p0, npl, only in rec:
        o = blob.h['OFF_COLL'] + int(c) * L.C['STRIDE']
        col = blob.collider(int(c))
        planes = cf[ci[L.CL['OFF_PLANE']] + 4 * p0:ci[L.CL['OFF_PLANE']] + 4 * (p0 + npl)].reshape(npl, 4).astype(np.float64)      # the padded repeat of the last plane included
        out.append(dict(collider=int(c), body=col['body'], radius=col['radius'], friction=col['friction'], verts=col['verts'], planes=planes, only=int(only),
                        aabb_c=blob.f[o + L.C['AABB_C']:o + L.C['AABB_C'] + 3].astype(np.float64), aabb_h=blob.f[o + L.C['AABB_H']:o + L.C['AABB_H'] + 3].astype(np.float64)))
    return out


def _quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def body_frames(blob, oracle, state, shapes):
    """world frame (p, R) of the body of every shape where the substep starts: moving links from the oracle's forward kinematics, the robot
    base and the human's static bodies from the state record"""
    pos, rot = oracle.fk(state)
    v = blob.view(state.reshape(1, -1))
    out = []
    for s in shapes:
        b = s['body']
        if b == L.BODY_WORLD:
            out.append((np.zeros(3), np.eye(3)))
        elif b >= L.BODY_HUMAN0:
            r = v['human'][0, b - L.BODY_HUMAN0].astype(np.float64)
            out.append((r[:3], _quat_to_mat(r[3:7])))
        elif b == L.BODY_ROBOT_BASE:
            r = v['base'][0].astype(np.float64)
            out.append((r[:3], _quat_to_mat(r[3:7])))
        else:
            out.append((pos[b].copy(), rot[b].copy()))
    return out


def _rel(a, b):
    """relative margin of the test a < b between two non-negative numbers"""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def _dot(a, b):
    """written out: the same bits on every machine (no BLAS), in the type of the operands"""
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _mv(R, v):
    return np.array([_dot(R[0], v), _dot(R[1], v), _dot(R[2], v)], dtype=v.dtype)


def shape_boxes(t, shapes, frames, dtype):
    """world box (lo, hi) of every shape: the core's body-frame box rotated into the world, grown by radius + margin + 1e-6 (float32 sum)"""
    F = np.dtype(dtype).type
    boxes = []
    for s, (p, R) in zip(shapes, frames):
        p, R = p.astype(dtype), R.astype(dtype)
        r = F(np.float32(s['radius']) + np.float32(t['par'][L.CP['MARGIN']]) + np.float32(1e-6))
        cw = p + _mv(R, s['aabb_c'].astype(dtype))
        hw = _mv(np.abs(R), s['aabb_h'].astype(dtype)) + r
        boxes.append((cw - hw, cw + hw))
    return boxes


def substep(t, shapes, frames, x, v, grav, dt, anchor, gender=0, dtype=np.float64, roundtrip=True, plant=None):
    """One internal substep of the garment, every number of type `dtype`.

    shapes / frames: shape_table / body_frames; gender: the state record's (0 male, 1 female).  In float32 mode with `roundtrip` the state
    record's round trip is applied as the kernel does: q = x - v dt / (1 - kDP) on load, v = (x - q) (1 - kDP) / dt on store.
    plant: one deliberate error (tests only), see test_cloth_kernel_cases.py.
    Returns x, v, contacts {(node, slot): |force|}, margins (dict of per-node arrays: the distance of every branch from its threshold;
    inf where the branch is not reached), info (nodes inside three or more margin shells, ...)."""
    F = np.dtype(dtype).type
    plant = plant or {}
    P = t['par']
    kLST, kDP, kDG, kDF, kCHR, kAHR, mrg, im, rho = (F(P[L.CP[k]]) for k in ('KLST', 'KDP', 'KDG', 'KDF', 'KCHR', 'KAHR', 'MARGIN', 'NODE_IM', 'AIR_DENSITY'))
    one, half, eps = F(1), F(0.5), F(EPS)
    dt, grav = F(dt), F(grav)
    nn = t['nn']
    x, v = np.array(x, dtype=dtype), np.array(v, dtype=dtype)
    area = t['area'].astype(dtype)
    anchor = np.asarray(anchor, dtype=dtype)
    M = {k: np.full(nn, np.inf) for k in ('dst', 'dn', 'friction', 'clamp', 'vn', 'plane')}
    if dtype == np.float32 and roundtrip:
        q = x - v * (dt / (one - kDP))
        v = ((one - kDP) / dt) * (x - q)
    # normals from the incident faces (every position read before any node moves), gravity, the one-sided drag and its clamp
    vn_ = v.copy()
    clamped = np.zeros(nn, dtype=bool)
    for i in range(nn):
        n = np.zeros(3, dtype=dtype)
        for e in range(t['node'][i], t['node'][i + 1]):
            j, k = t['face'][e] & 0xffff, (t['face'][e] >> 16) & 0xffff
            n = n + np.cross(x[j] - x[i], x[k] - x[i]).astype(dtype)
        ln = np.sqrt(_dot(n, n))
        if ln > eps:
            n = n * (one / ln)
        vi = v[i].copy()
        vi[2] = vi[2] + grav * dt
        s2 = _dot(vi, vi)
        if kDG > 0 and s2 > eps:
            dvn = _dot(vi, n)
            M['vn'][i] = abs(float(dvn))
            if dvn > 0:
                f = area[i] * dvn * s2 * half * rho * kDG            # magnitude of the drag, against the velocity
                dtim = dt * im
                M['clamp'][i] = _rel(float(f * dtim) ** 2, float(s2))
                if f * dtim * f * dtim > s2:
                    vi = np.zeros(3, dtype=dtype)
                    clamped[i] = True
                else:
                    vi = vi - (f * dtim / np.sqrt(s2)) * vi
        vn_[i] = vi
    q = x.copy()
    x = q + dt * vn_
    # contacts: per node the first NODE_CONTACTS shapes, in shape order, whose margin shell holds the node
    anchored = set(int(a) for a in t['anchors'])
    boxes = shape_boxes(t, shapes, frames, dtype)
    contacts = {}
    shells = np.zeros(nn, dtype=int)
    for i in range(nn):
        if i in anchored and not plant.get('anchored_collide'):
            continue
        found = []
        for sh, (s, (p, R)) in enumerate(zip(shapes, frames)):
            if s['only'] and s['only'] != gender + 1:
                continue
            lo, hi = boxes[sh]
            if (x[i] < lo).any() or (x[i] > hi).any():
                continue
            p, R = p.astype(dtype), R.astype(dtype)
            xl = _mv(R.T, x[i] - p)
            rad = F(s['radius'])
            plane_gap = np.inf
            if len(s['planes']) == 0:
                a = s['verts'][0].astype(dtype)
                b = s['verts'][1].astype(dtype) if len(s['verts']) == 2 else a
                ab, ax = b - a, xl - a
                l2 = _dot(ab, ab)
                u = _dot(ax, ab) / l2 if l2 > 0 else F(0)
                u = min(max(u, F(0)), one)
                nl = xl - (a + u * ab)
                ln = np.sqrt(_dot(nl, nl))
                nl = nl * (one / ln) if ln > 1e-12 else np.array([0, 0, 1], dtype=dtype)
                dist = ln - rad
            else:
                pl = s['planes'].astype(dtype)
                if plant.get('negate_plane') is not None and plant['negate_plane'][0] == sh:
                    pl = pl.copy(); pl[plant['negate_plane'][1], :3] *= -1
                tt = pl[:, 0] * xl[0] + pl[:, 1] * xl[1] + pl[:, 2] * xl[2] - pl[:, 3]
                best = int(np.argmax(tt))                            # ties keep the first
                other = tt[np.any(pl != pl[best], axis=1)]
                if len(other):
                    plane_gap = float(tt[best] - other.max())
                nl, dist = pl[best, :3], tt[best] - rad
            nw = _mv(R, nl)
            dst = dist - mrg
            M['dst'][i] = min(M['dst'][i], abs(float(dst)))
            if dst >= 0:
                continue
            shells[i] += 1
            if len(s['planes']):                                      # a hull's plane distance can accept points beyond the box: the box decides too
                M['dst'][i] = min(M['dst'][i], float(np.minimum(x[i] - lo, hi - x[i]).min()))
                if len(found) < NODE_CONTACTS:
                    M['plane'][i] = min(M['plane'][i], plane_gap)
            found.append((sh, nw, dst, s['friction']))
        if plant.get('third_contact') and len(found) > NODE_CONTACTS:
            found = [found[0], found[2]]
        for slot, (sh, nw, dst, fr) in enumerate(found[:NODE_CONTACTS]):
            vr = x[i] - q[i]
            dn = _dot(vr, nw)
            fv = vr - dn * nw
            fc = kDF * F(fr)
            M['friction'][i] = min(M['friction'][i], _rel(float(_dot(fv, fv)), float(dn * fc * dn * fc)))
            stick = _dot(fv, fv) < dn * fc * dn * fc
            c3 = (one - fc) if (not stick or plant.get('friction')) else F(0)
            contacts[(i, slot)] = dict(n=nw, off=-_dot(nw, x[i]) + dst, c3=c3, imp=np.zeros(3, dtype=dtype), sh=sh)
    # position solver: anchors, rigid contacts, links class by class
    order = list(range(t['ncolor']))
    if plant.get('swap_classes') is not None:
        c = plant['swap_classes']
        order[c], order[c + 1] = order[c + 1], order[c]
    keep = np.ones(len(t['a']), dtype=bool)
    if plant.get('drop_link') is not None:
        keep[plant['drop_link']] = False
    cls_links = [np.nonzero((t['cls'] == c) & keep)[0] for c in range(t['ncolor'])]
    rest2 = t['rest2'].astype(dtype)
    w = one / (dt * im)
    for it in range(int(P[L.CP['PITER']])):
        for a, i in enumerate(t['anchors']):
            wa = anchor + t['anchor_off'][a].astype(dtype)
            x[i] = x[i] + F(-1) * (x[i] - q[i]) + kAHR * (wa - x[i])
        for (i, slot), c in contacts.items():
            vr = x[i] - q[i]
            dn = _dot(vr, c['n'])
            M['dn'][i] = min(M['dn'][i], abs(float(dn) - EPS))
            if dn <= eps:
                dp = min(_dot(x[i], c['n']) + c['off'], mrg)
                fv = vr - dn * c['n']
                corr = vr - c['c3'] * fv + (dp * kCHR) * c['n']
                x[i] = x[i] - corr
                c['imp'] = c['imp'] + w * corr
        for c in order:                         # the links of a class share no node: relaxing them at once is relaxing them in any order
            ls = cls_links[c]
            if len(ls) == 0:
                continue
            a, b = t['a'][ls], t['b'][ls]
            d = x[b] - x[a]
            ln = (d * d).sum(1).astype(dtype)
            c1 = rest2[ls]
            ok = c1 + ln > eps
            k = np.where(ok, (c1 - ln) / np.where(ok, c1 + ln, one) * kLST * half, F(0)).astype(dtype)
            x[a] = x[a] - k[:, None] * d
            x[b] = x[b] + k[:, None] * d
    v = ((x - q) * ((one - kDP) / dt)) if dtype == np.float32 else (x - q) / dt * (one - kDP)
    force = {}
    for (i, slot), c in contacts.items():
        f = (one / dt) * c['imp']
        force[(i, slot)] = float(np.sqrt(_dot(f, f)))
    if plant.get('slot1_to_slot0'):
        force = {(i, 0): f for (i, slot), f in force.items() if slot == 1 or (i, 1) not in force}
    assert x.dtype == dtype and v.dtype == dtype
    return x, v, force, M, dict(shells=shells, q=q, clamped=clamped)


def determined(M, band=BAND):
    return all((M[k] >= band[k]).all() for k in band)


def free_flight(t, shapes, frames, x, v, grav, anchor, dtype, n_sub=8, dt=0.02 / 8, plant=None):
    """one stepSimulation of a garment out of reach of every shape (asserted: no node enters a shape's box; `frames` are those of the first
    substep): n_sub substeps, the state record's round trip once.  Returns x, v and the smallest margin of the drag clamp (the one
    discontinuous branch of free flight: the one-sided drag vanishes at its own threshold) with the number of nodes it stopped."""
    clamp, fired = np.inf, 0
    for k in range(n_sub):
        x, v, con, M, info = substep(t, shapes, frames, x, v, grav, dt, anchor, dtype=dtype, roundtrip=k == 0, plant=plant)
        assert not con and np.isinf(M['dst']).all(), 'a node came within reach of a shape'
        clamp = min(clamp, float(M['clamp'].min()))
        fired += int(info['clamped'].sum())
    return x, v, clamp, fired


# ---------------------------------------------------------------------------------------------------- judging a result
def ulp32(a):
    """one float32 ulp of the largest coordinate magnitude in a"""
    return float(np.spacing(np.float32(np.abs(a).max())))


def limits(dev_x, dev_v, dev_f, x, dt, im, factor=4.0):
    """Limits of a comparison against a float64 result: `factor` x the float32 restatement's own deviation from it (an independent float32
    evaluation of the same arithmetic; the device may differ from it by summation order and FMA contraction), with a floor of one float32 ulp
    of the coordinate magnitude for x, that ulp / dt for v (v = (x - q) (1 - kDP) / dt) and that ulp / (dt^2 im) for a contact force (the sum
    of the position corrections of the substep / (dt^2 im))."""
    u = ulp32(x)
    return dict(x=max(factor * dev_x, u), v=max(factor * dev_v, u / dt), f=max(factor * dev_f, u / (dt * dt * im)))


def report_contacts(report, nn):
    """{(node, slot): |force|} from one environment's cloth report (agx_get_cloth_report): 20 words, then {node height, |force| or -1} per node and slot"""
    r = np.asarray(report)[20:20 + 2 * NODE_CONTACTS * nn].reshape(nn, NODE_CONTACTS, 2)
    return {(int(i), int(s)): float(r[i, s, 1]) for i, s in zip(*np.nonzero(r[:, :, 1] >= 0))}, r[:, :, 0]


def compare(x, v, contacts, want_x, want_v, want_contacts, lim, heights=None):
    """A result (x, v float32 [NN, 3], contacts {(node, slot): |force|}) against the float64 one on ALL nodes: maxima, not percentiles, and the
    contact set exactly.  Returns (measured maxima, list of violations -- empty: accepted)."""
    m = dict(x=float(np.abs(np.asarray(x, dtype=np.float64) - want_x).max()), v=float(np.abs(np.asarray(v, dtype=np.float64) - want_v).max()), f=0.0, contacts=len(want_contacts))
    bad = []
    if not (np.isfinite(x).all() and np.isfinite(v).all()):
        bad.append('not finite')
    if set(contacts) != set(want_contacts):
        bad.append('contact set differs: missing %s, extra %s' % (sorted(set(want_contacts) - set(contacts))[:5], sorted(set(contacts) - set(want_contacts))[:5]))
    else:
        m['f'] = max([abs(contacts[k] - want_contacts[k]) for k in want_contacts] + [0.0])
        if heights is not None:
            for (i, s) in want_contacts:
                if abs(heights[i, s] - want_x[i, 2]) > lim['x']:
                    bad.append('report height of node %d slot %d' % (i, s))
    for k in ('x', 'v', 'f'):
        if not m[k] <= lim[k]:
            bad.append('%s: %.3g beyond %.3g' % (k, m[k], lim[k]))
    return m, bad


# ---------------------------------------------------------------------------------------------------- the stored cases
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cloth_kernel_cases.npz')
DT = 0.02 / 8
_CACHE = {}


def load_cases():
    """tests/golden/cloth_kernel_cases.npz (tests/diag/make_cloth_kernel_cases.py) as a dict; recipes decoded"""
    if 'cases' not in _CACHE:
        import json
        z = np.load(GOLDEN)
        _CACHE['cases'] = {k: (json.loads(str(z[k])) if k.endswith('/recipe') else z[k]) for k in z.files}
    return _CACHE['cases']


def case_blob(rec):
    """the spliced blob of a stored case, from its recipe (one per recipe and process: compiling the 4,096-node garment takes seconds)"""
    from assistive_gym_amd.blob import ModelBlob
    key = repr((rec['grid'], rec['spacing'], rec['anchors'], rec['shape_ids'], sorted(rec['overrides'].items())))
    if key not in _CACHE:
        nx, ny = rec['grid']
        _CACHE[key] = splice(ModelBlob.load('dressing_baxter'), nx, ny, rec['spacing'], anchors=rec['anchors'], shape_ids=rec['shape_ids'], overrides=rec['overrides'])
    return _CACHE[key]


def free_input(t, rec):
    """the garment of a free-flight case from its recipe: rest positions lifted above the end effector, seeded node velocities"""
    x = t['x0'] + np.asarray(rec['ee']) + np.array([0, 0, rec['lift']])
    v = np.random.RandomState(rec['seed']).uniform(-rec['speed'], rec['speed'], x.shape)
    v[:, 2] -= 0.5
    return x.astype(np.float32), v.astype(np.float32)


def forced_substeps(cases, name, determined_only=True):
    """the stored substeps of a forced scene: dicts of state record, input garment, float64 result (x, v), contacts {(node, slot): |force|}"""
    out = []
    con, force = cases[name + '/con'], cases[name + '/force']
    for k in range(len(cases[name + '/sub'])):
        if determined_only and not cases[name + '/det'][k]:
            continue
        xin = cases[name + '/xin'][k]
        m = con[:, 0] == k
        out.append(dict(sub=int(cases[name + '/sub'][k]), det=bool(cases[name + '/det'][k]), state=cases[name + '/state'][k], xin=xin, vin=cases[name + '/vin'][k],
                        x=xin.astype(np.float64) + cases[name + '/dx'][k].astype(np.float64), v=cases[name + '/v'][k].astype(np.float64),
                        con={(int(i), int(s)): float(f) for (_, i, s), f in zip(con[m], force[m])}))
    return out


def forced_limits(cases, name, blob):
    """the limits of a forced scene: from the float32 restatement's deviation in its stored determined substeps"""
    det = cases[name + '/det']
    dev = cases[name + '/dev'][det].max(0)
    x = cases[name + '/xin'][det]
    im = float(tables(blob)['par'][L.CP['NODE_IM']])
    return limits(dev[0], dev[1], dev[2], x, DT, im)


def judge_forced(cases, name, blob, results):
    """results: per stored determined substep (x, v, contacts, heights or None).  Returns (maxima over the scene, violations)."""
    lim = forced_limits(cases, name, blob)
    subs = forced_substeps(cases, name)
    assert len(results) == len(subs)
    tot, bad = dict(x=0.0, v=0.0, f=0.0, contacts=0), []
    for want, (x, v, con, heights) in zip(subs, results):
        m, b = compare(x, v, con, want['x'], want['v'], want['con'], lim, heights)
        bad += ['substep %d: %s' % (want['sub'], t) for t in b]
        for k in ('x', 'v', 'f'):
            tot[k] = max(tot[k], m[k])
        tot['contacts'] += m['contacts']
    return tot, lim, bad


def judge_free(cases, name, t, x, v):
    rec = cases[name + '/recipe']
    xin, _ = free_input(t, rec)
    want_x = xin.astype(np.float64) + cases[name + '/dx'].astype(np.float64)
    dev = cases[name + '/dev']
    lim = limits(dev[0], dev[1], 0.0, want_x, DT, float(t['par'][L.CP['NODE_IM']]))
    m, bad = compare(x, v, {}, want_x, cases[name + '/v'].astype(np.float64), {}, lim)
    return m, lim, bad
