"""Writes tests/golden/cloth_kernel_cases.npz: the node-exact cases of tests/test_cloth_kernel_cases.py (CPU) and tests/test_gpu_cloth_kernel.py.

Small synthetic garments (tests/cloth_cases.py) spliced into the DressingBaxter blob, one seeded state record, and per case the float64 result
of the numpy restatement together with the float32 restatement's own deviation from it -- what the device's limits are made of.

  free flight (ff_*)    no shape in reach, one stepSimulation of 8 substeps, random node velocities; scenes A (6 x 5, anchors at KAHR 1 and
                        0), B (17 x 16), C (40 x 26), D (64 x 64 at 12 mm); two of them with a drag strong enough that the clamp stops some
                        nodes and not others.  The garment is rebuilt from the stored recipe (rest positions, offset, seed): no input array.
  forced substeps (fs_*) a patch on the forearm capsule (sliding, dropped; scenes A and B), on a wheelchair hull, in the overlap of upper arm,
                        elbow and forearm (the two-contact cap decides), and under a shape list that holds the female forearm with a male
                        record.  No node RESTS inside three shells (the two kept contacts push it out of theirs), so the overlap scene is no
                        trajectory: each of its substeps starts from a placement of its own, moving into the shells.  Elsewhere every
                        substep starts from the float64 run's own state rounded to float32 (teacher forcing) and from the
                        rigid scene advanced by the one-substep oracle; a substep is DETERMINED when every branch of every node is clear of
                        its threshold by the bands of cloth_cases.BAND.  Stored: the determined substeps (at most KEEP) and a few others for
                        the oracle-against-restatement test.

Sizes: x is stored as float64 through (float32 input, float32 difference to it) -- the difference is a millimetre, its rounding 1e-10 m; v as
float32 (rounding 6e-8 m/s against a floor of one ulp of a coordinate / dt = 2e-5 m/s).
The stored force deviation of the float32 restatement includes the shapes' frames moved by one float32 ulp (see run_forced).
Not a test; run by hand:  python tests/diag/make_cloth_kernel_cases.py     (CPU only, about two minutes)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cloth_cases as CC
from assistive_gym_amd.model import compiler as L

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'cloth_kernel_cases.npz')
GRID = dict(A=(6, 5, 0.03), B=(17, 16, 0.03), C=(40, 26, 0.03), D=(64, 64, 0.012), E=(8, 8, 0.012))      # E: a dense patch for the overlap scene
DT = 0.02 / 8
GRAVITY = -9.81
KEEP = 10           # determined substeps stored per forced scene
KEEP_OTHER = 2      # ... and undetermined ones (scene A size only)

FREE = dict(
    ff_A_k1=dict(scene='A', overrides={}, speed=0.5, lift=0.02),
    ff_A_k0_clamp=dict(scene='A', overrides=dict(KAHR=0.0, KDG=100.0), speed=1.0, lift=0.3),
    ff_B=dict(scene='B', overrides={}, speed=0.5, lift=0.02),
    ff_C_clamp=dict(scene='C', overrides=dict(KDG=100.0), speed=1.0, lift=0.02),
    ff_D=dict(scene='D', overrides=dict(KAHR=0.0), speed=0.5, lift=0.6),
)
# shapes by role (resolved against the blob's collider ranges in resolve_shapes); `at`: what the patch is centred over; `v0`: initial velocity
FORCED = dict(
    fs_A_slide=dict(scene='A', shapes=['forearm'], at='forearm', v0=(0.05, 0.0, 0.0), n_sub=80),
    fs_A_drop=dict(scene='A', shapes=['forearm'], at='forearm', v0=(0.0, 0.0, -0.5), n_sub=80),
    fs_B_slide=dict(scene='B', shapes=['forearm'], at='forearm', v0=(0.05, 0.0, 0.0), n_sub=80),
    fs_B_drop=dict(scene='B', shapes=['forearm'], at='forearm', v0=(0.0, 0.0, -0.5), n_sub=80),
    fs_hull=dict(scene='A', shapes=['hull'], at='hull', v0=(0.05, 0.0, 0.0), n_sub=80),
    # nodes on the forearm next to the elbow are inside the elbow's and the upper arm's shells as well: the cap keeps the first two.  (The upper arm's
    # capsule ends in the elbow's centre with the elbow's radius: there its contact IS the elbow's, so it comes last -- kept in the forearm's place it shows)
    fs_overlap=dict(scene='E', shapes=['elbow', 'forearm', 'upperarm'], at='elbow', offset=(-0.01, -0.02, 0.0), v0=(0.05, 0.0, -0.2), reseat=(0.0002, 0.0, -0.0003), n_sub=80),
    # ... hung by its two middle nodes, which lie inside the forearm's shell and must not collide
    fs_gender=dict(scene='A', shapes=['forearm_female', 'forearm'], at='forearm', anchors='centre', v0=(0.05, 0.0, 0.0), n_sub=80),
    # arriving: the whole patch above the forearm's box where the substep starts, its lowest node inside the margin shell after the prediction (the
    # shell touches its box along the top line of this horizontal capsule) -- the contact exists in the substep in which the node arrives, not one
    # later.  One placement per substep, 0.1 mm higher each time; one contact each.
    fs_first_touch=dict(scene='A', shapes=['forearm'], at='box_top', v0=(0.0, 0.0, -0.5), reseat=(0.0, 0.0, 0.0001), n_sub=12),
)
MIN_CONTACTS = dict(fs_first_touch=10)      # (every other forced scene: 50)
HEIGHTS = (0.035, 0.03, 0.025, 0.02)      # of the patch's mean above the shape's surface: the first that meets the scene's conditions


def load():
    from assistive_gym_amd.blob import ModelBlob
    return ModelBlob.load('dressing_baxter')


def record(dr, seed=71):
    """one seeded post-reset state record (a male without impairment), the garment's gravity at its episode value"""
    from assistive_gym_amd.host.reset_dressing import DressingBaxterReset
    st = dr.new_state(1)
    cl = np.zeros((2, 3966, 3), dtype=np.float32)
    DressingBaxterReset(dr).sample(np.random.RandomState(seed), st, cl, env_seed=seed, gender='male', impairment='none')
    dr.view(st)['task'][0, L.DR['CLOTH_GRAVITY']] = np.array([GRAVITY], dtype=np.float32).view(np.int32)[0]
    return st[0]


def resolve_shapes(dr, roles):
    fa = CC.forearm_capsule(dr)
    by_link = lambda g, link, nv: [c for c in range(*dr.meta['ranges']['human_' + g]) if dr.collider(c)['link'] == link and len(dr.collider(c)['verts']) == nv][0]
    table = dict(forearm=fa, forearm_female=CC.forearm_capsule(dr, 'female'), elbow=by_link('male', 16, 1), upperarm=by_link('male', 15, 2),
                 hull=dr.meta['ranges']['wheelchair'][0] + 1)      # the wheelchair's left arm rest: 22 vertices
    return [table[r] for r in roles]


def scene_blob(dr, scene, shape_ids, overrides, anchors=None):
    nx, ny, h = GRID[scene]
    return CC.splice(dr, nx, ny, h, anchors=anchors or (0, nx - 1), shape_ids=shape_ids, overrides=overrides)


def make_free(dr, state, name, log=print):
    from oracle_lib import Oracle
    rec = dict(FREE[name])
    shape_ids = resolve_shapes(dr, ['forearm'])
    blob = scene_blob(dr, rec['scene'], shape_ids, rec['overrides'])
    o = Oracle(blob)
    t, shapes = CC.tables(blob), CC.shape_table(blob)
    frames = CC.body_frames(blob, o, state, shapes)
    ee, _ = o.ee_pose(state)
    want_clamp = 'clamp' in name
    for seed in range(3, 40):
        rec['seed'] = seed
        x, v = CC.free_input(t, dict(rec, ee=ee))
        x64, v64, clamp, fired = CC.free_flight(t, shapes, frames, x.astype(np.float64), v.astype(np.float64), GRAVITY, ee, np.float64)
        if clamp < CC.BAND['clamp'] or (want_clamp and not 0 < fired):
            continue
        x32, v32, _, fired32 = CC.free_flight(t, shapes, frames, x, v, GRAVITY, ee, np.float32)
        assert fired32 == fired
        break
    else:
        raise RuntimeError(name + ': no seed with the drag clamp clear of its threshold')
    dev = np.array([np.abs(x32 - x64).max(), np.abs(v32 - v64).max()])
    nx, ny, h = GRID[rec['scene']]
    rec.update(grid=[nx, ny], spacing=h, anchors=[0, nx - 1], shape_ids=shape_ids, ee=[float(e) for e in ee], nodes=t['nn'], clamp_fired=fired,
               cross_classes=t['ncolor'] - t['first_cross'])
    log('%s: seed %d, %d nodes, %d cross classes, clamp stopped %d node-substeps (margin %.2e), float32 deviation x %.2e v %.2e' % (name, seed, t['nn'], rec['cross_classes'], fired, clamp, dev[0], dev[1]))
    return {name + '/recipe': np.array(json.dumps(rec)), name + '/dx': (x64 - x.astype(np.float64)).astype(np.float32), name + '/v': v64.astype(np.float32), name + '/dev': dev}


def run_forced(dr, state, name, height, log=print):
    from oracle_lib import Oracle
    rec = dict(FORCED[name])
    shape_ids = resolve_shapes(dr, rec['shapes'])
    blob1 = CC.one_substep_blob(scene_blob(dr, rec['scene'], shape_ids, dict(KAHR=0.0), rec.get('anchors')))      # hardness 0 pins the anchored nodes where they are
    o1 = Oracle(blob1)
    t, shapes = CC.tables(blob1), CC.shape_table(blob1)
    s = state.copy()
    frames = CC.body_frames(blob1, o1, s, shapes)
    k = rec['shapes'].index({'elbow': 'elbow', 'hull': 'hull'}.get(rec['at'], 'forearm'))
    p, R = frames[k]
    if rec['at'] == 'hull':          # across the long edge of the arm rest's top face: nodes over the face, over the edge and beyond it
        w = p + shapes[k]['verts'] @ R.T
        top = np.array([w[:, 0].max() - 0.03, 0.5 * (w[:, 1].min() + w[:, 1].max()), w[:, 2].max()])
    else:
        top = p + R @ shapes[k]['verts'].mean(0)
    if rec['at'] == 'box_top':       # the lowest node nearest the patch's middle straight above the capsule's axis, 0.1 mm above the shape's box
        lo, hi = CC.shape_boxes(t, shapes, frames, np.float64)[k]
        low = np.nonzero(t['x0'][:, 2] == t['x0'][:, 2].min())[0]
        c = low[np.argmin(np.linalg.norm(t['x0'][low, :2] - t['x0'][:, :2].mean(0), axis=1))]
        top = np.array([top[0], top[1], hi[2] + 0.0001]) - (t['x0'][c] - t['x0'].mean(0)) - np.array([0, 0, shapes[k]['radius'] + height])

    def place(sub):
        x = t['x0'] - t['x0'].mean(0) + top + np.array(rec.get('offset', (0.0, 0.0, 0.0))) + np.array([0, 0, shapes[k]['radius'] + height]) + sub * np.array(rec.get('reseat', (0.0, 0.0, 0.0)))
        v = np.zeros_like(x) + np.array(rec['v0'])
        return x.astype(np.float32), v.astype(np.float32)
    x, v = place(0)
    rows = []
    for sub in range(rec['n_sub']):
        frames = CC.body_frames(blob1, o1, s, shapes)
        anchor, _ = o1.ee_pose(s)
        x64, v64, f64, M, info = CC.substep(t, shapes, frames, x.astype(np.float64), v.astype(np.float64), GRAVITY, DT, anchor, gender=0, dtype=np.float64)
        x32, v32, f32, _, _ = CC.substep(t, shapes, frames, x, v, GRAVITY, DT, anchor, gender=0, dtype=np.float32)
        det = CC.determined(M)
        same = set(f32) == set(f64)
        assert same or not det, (name, sub, 'the float32 restatement found other contacts in a determined substep')
        dev = [np.abs(x32 - x64).max(), np.abs(v32 - v64).max(), max([abs(f32[c] - f64[c]) for c in f64] + [0.0]) if same else np.inf]
        if det:      # a contact force answers to the shape's position with 1 / (dt^2 im) = 6.5 N/m, and that position is itself a float32 result (the
            # rigid kernels' forward kinematics): the float32 restatement's force deviation is taken over the frames rounded to nearest and moved
            # by one float32 ulp either way.  x and v keep the deviation of the nearest frames.
            for way in (np.inf, -np.inf):
                moved = [(np.nextafter(p.astype(np.float32), np.float32(way)).astype(np.float64), R) for p, R in frames]
                fm = CC.substep(t, shapes, moved, x, v, GRAVITY, DT, anchor, gender=0, dtype=np.float32)[2]
                assert set(fm) == set(f64), (name, sub)
                dev[2] = max([dev[2]] + [abs(fm[c] - f64[c]) for c in f64])
        if rec['at'] == 'box_top':
            lo, hi = CC.shape_boxes(t, shapes, frames, np.float64)[0]
            assert x[:, 2].min() > hi[2] and f64, 'not a first touch'
        rows.append(dict(sub=sub, det=det, state=s.copy(), xin=x, vin=v, x=x64, v=v64, con=f64, dev=dev, triple=int((info['shells'] >= 3).sum()), why=[k for k in CC.BAND if not (M[k] >= CC.BAND[k]).all()]))
        o1.settle(s, 1)
        x, v = x64.astype(np.float32), v64.astype(np.float32)
        if 'reseat' in rec:          # no trajectory: every substep starts from a placement of its own, `reseat` further on than the one before
            x, v = place(sub + 1)
    nx, ny, h = GRID[rec['scene']]
    rec.update(grid=[nx, ny], spacing=h, anchors=rec.get('anchors') or [0, nx - 1], shape_ids=shape_ids, overrides=dict(KAHR=0.0), height=height, nodes=t['nn'])
    return rec, rows


def kept(rows):
    """the determined substeps that go into the fixture: those with the most contacts"""
    det = sorted([r for r in rows if r['det']], key=lambda r: (-len(r['con']), r['sub']))[:KEEP]
    return sorted(det, key=lambda r: r['sub'])


def conditions(name, rows):
    keep = kept(rows)
    det = [r for r in rows if r['det']]
    msg = []
    if len(det) < 10:
        msg.append('%d determined substeps' % len(det))
    if sum(len(r['con']) for r in keep) < MIN_CONTACTS.get(name, 50):
        msg.append('%d contacts' % sum(len(r['con']) for r in keep))
    if len(rows) - len(det) > 0.75 * len(rows):
        msg.append('%d of %d substeps left out' % (len(rows) - len(det), len(rows)))
    if name == 'fs_overlap' and max([r['triple'] for r in keep] + [0]) < 5:
        msg.append('at most %d nodes inside three shells' % max([r['triple'] for r in keep] + [0]))
    return msg


def make_forced(dr, state, name, log=print):
    for height in HEIGHTS:
        rec, rows = run_forced(dr, state, name, height, log)
        msg = conditions(name, rows)
        if not msg:
            break
        log('%s at %.3f m: %s -- next placement (undetermined by band: %s)' % (name, height, ', '.join(msg), {k: sum(k in r['why'] for r in rows) for k in CC.BAND}))
    else:
        raise RuntimeError(name + ': no placement meets the conditions')
    det = kept(rows)
    other = [r for r in rows if not r['det']][:KEEP_OTHER if rec['nodes'] <= 64 else 0]
    keep = sorted(det + other, key=lambda r: r['sub'])
    con = np.array([(k, i, s) for k, r in enumerate(keep) for (i, s) in sorted(r['con'])], dtype=np.int16).reshape(-1, 3)
    force = np.array([r['con'][c] for r in keep for c in sorted(r['con'])])
    mask = np.array([r['det'] for r in rows])
    dev = np.array([r['dev'] for r in keep])
    kdet = np.array([r['det'] for r in keep])
    rec.update(determined=int(mask.sum()), left_out=int((~mask).sum()), contacts_compared=int(sum(len(r['con']) for r in det)), triple_nodes=int(max([r['triple'] for r in det] + [0])))
    log('%s at %.3f m: %d of %d substeps determined, %d stored (%d determined, %d contacts, up to %d nodes in three shells); float32 deviation in them x %.2e v %.2e f %.2e; in the others x %.2e'
        % (name, rec['height'], mask.sum(), len(rows), len(keep), len(det), rec['contacts_compared'], rec['triple_nodes'], dev[kdet, 0].max(), dev[kdet, 1].max(), dev[kdet, 2].max(),
           max([r['dev'][0] for r in rows if not r['det']] + [0.0])))
    xin = np.array([r['xin'] for r in keep])
    return {name + '/recipe': np.array(json.dumps(rec)), name + '/mask': mask, name + '/sub': np.array([r['sub'] for r in keep], dtype=np.int16), name + '/det': kdet,
            name + '/state': np.array([r['state'] for r in keep]), name + '/xin': xin, name + '/vin': np.array([r['vin'] for r in keep]),
            name + '/dx': np.array([r['x'] for r in keep] - xin.astype(np.float64)).astype(np.float32), name + '/v': np.array([r['v'] for r in keep]).astype(np.float32),
            name + '/con': con, name + '/force': force, name + '/dev': dev}


def make(names=None, log=print):
    dr = load()
    state = record(dr)
    out = dict(state=state)
    for name in (names or list(FREE) + list(FORCED)):
        out.update(make_free(dr, state, name, log) if name in FREE else make_forced(dr, state, name, log))
    return out


def main():
    out = make()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
