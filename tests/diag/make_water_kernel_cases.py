"""Writes tests/golden/water_kernel_cases.npz: the particle-exact cases of tests/test_water_kernel_cases.py (CPU) and tests/test_gpu_water_kernel.py.

Small synthetic waters (tests/water_cases.py) spliced into the DrinkingJaco blob, the settled state record of tests/test_drinking.py (seed 3),
and per scene a sequence of FORCED substeps: the state record is fixed, the water evolves under the float64 numpy restatement (every substep
starts from the float64 result rounded to float32) or -- where a trajectory leaves the situation the scene is about -- every substep starts
from a placement of its own (`place`, seeded).  A substep is DETERMINED when every branch of every particle is clear of its threshold by the
bands of water_cases.BAND.  Stored per scene: the recipe, and per stored substep the state record, the input water, the float64 result (x as a
float32 difference to the float32 input, v as float32), the hits {(particle, shape)}, the determined flag and the float32 restatement's own
deviation from the float64 result -- what the device's limits are made of.  Where a shape sits on a moving link or on the cup (the device's
frames then come from float32 forward kinematics) that deviation is the largest over the frames rounded to float32 and moved one float32 ulp
either way.  ww_hit_last is a LAUNCH of the ordinary four-substep blob over the frames of the oracle's trace hook.

Scenes: see SCENES below and profiles/water_kernel_tests/README.md.
Not a test; run by hand:  python tests/diag/make_water_kernel_cases.py     (CPU only, a few minutes)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import water_cases as WC
from assistive_gym_amd.model import compiler as L

OUT = WC.GOLDEN
KEEP = 10           # determined substeps stored per scene
KEEP_OTHER = 2      # ... and undetermined ones, for the oracle-against-restatement test (none in ww_cup_rest)
R = 0.005


def load():
    from assistive_gym_amd.blob import ModelBlob
    return ModelBlob.load('drinking_jaco')


def settled(dk):
    """the settled state record and water of tests/test_drinking.py's `settled` fixture"""
    from assistive_gym_amd.host.reset_drinking import make_states
    from oracle_lib import Oracle
    st, water, infos = make_states(dk, 1, seed=3, impairment='none')
    s, w = st[0].copy(), water[0].copy()
    Oracle(dk).settle_cloth(s, w, 50)
    return s, w


class World:
    """the colliders of the person (of the record's gender), the cup and the rest by role, and where they are in the settled state"""
    def __init__(self, dk, state):
        from oracle_lib import Oracle
        self.dk, self.state = dk, state
        self.gender = int(dk.view(state[None])['gender'][0])
        self.frames = WC.body_frames(dk, state, WC.moving_of_state(dk, Oracle(dk), state))
        self.r = dk.meta['ranges']

    def person(self, body, gender=None):
        g = self.gender if gender is None else gender
        return [c for c in range(*self.r['human_' + ('male', 'female')[g]]) if self.dk.collider(c)['body'] == body][0]

    def ends(self, c):
        col = self.dk.collider(c)
        p, Rm = self.frames[col['body']]
        return [p + Rm @ v for v in col['verts']], col['radius']

    def on_capsule(self, c, u, direction, gap):
        """the point at parameter u of capsule c's axis, moved along `direction` (made perpendicular to the axis) so that a particle of
        radius R there has `gap` between its surface and the capsule's"""
        (a, b), rad = self.ends(c)
        ax = (b - a) / np.linalg.norm(b - a)
        d = np.asarray(direction, dtype=np.float64)
        d = d - ax * (d @ ax)
        d /= np.linalg.norm(d)
        return a + u * (b - a) + d * (rad + R + gap), d, ax


SHOULDER_L, SHOULDER_R, FOREARM_L, HAND_L, FOREARM_R, HAND_R, HEAD, THIGH_L, THIGH_R = 301, 305, 303, 304, 307, 308, 10, 311, 314      # body codes


def _scene(x0, shape_ids, overrides=None, keep_planes=None, friction=None, radius=R, nsub=1):
    return dict(splice=dict(x0=np.round(np.asarray(x0, dtype=np.float64), 6).tolist(), radius=radius, shape_ids=[int(c) for c in shape_ids], overrides=overrides or {},
                            keep_planes={str(k): int(n) for k, n in (keep_planes or {}).items()}, friction={str(k): float(f) for k, f in (friction or {}).items()}), nsub=nsub)


# ---------------------------------------------------------------------------------------------------- the scenes
# each builder returns (recipe, states [per placement or one], place(k) -> (x, v) float32, n tried, evolve?, conditions(rows) -> list of complaints)
def ww_free(W, nn):
    """no shape in reach (the full shape list of the drinking scene, 179 shapes, none near): nn particles a metre above the cup with seeded
    velocities; up to two of them parked beyond 500 m (the "drunk" ones of drinking.py:70), which fall like the others and meet nothing --
    although, from two particles on, the state record puts the person's right hand (a static body) out there under the first parked one,
    which moves into it: beyond 500 m a particle has no candidates, whatever is there"""
    dk = W.dk
    ids = [s['collider'] for s in WC.shape_table(dk)]
    rs = np.random.RandomState(100 + nn)
    cup = dk.view(W.state[None])['free'][0, 0, :3].astype(np.float64)
    x = cup + [0, 0, 1.0] + rs.uniform(-0.1, 0.1, (nn, 3))
    v = rs.uniform(-0.5, 0.5, (nn, 3))
    parked = [nn - 1, nn // 2][:max(0, min(2, nn - 1))]
    for j, i in enumerate(parked):
        x[i] = [1000.0 + 7 * j, -2000.0, 3000.0 - j]
    state = W.state.copy()
    if parked:
        hand = W.person(HAND_R)
        dk.view(state[None])['human'][0, HAND_R - L.BODY_HUMAN0, :3] = [600.0, -700.0, 800.0]
        (c,), rad = World(dk, state).ends(hand)
        x[parked[0]], v[parked[0]] = c + [0, 0, rad + R + 2e-4], [0.0, 0.0, -0.3]
    rec = _scene(np.zeros((nn, 3)), ids, dict(KDP=0.01))
    rec['parked'] = parked

    def cond(rows):
        return [] if all(not r['hits'] and (r['info']['ncand'] == 0).all() and sorted(np.nonzero(~r['info']['here'])[0]) == sorted(parked) for r in rows) else ['a shape in reach']
    return rec, [state], lambda k: (x.astype(np.float32), v.astype(np.float32)), 12, True, cond


def ww_pile(W):
    """no shapes at all.  Particles 1, 2: a pair that overlaps (cnt = 1: no division); 3-5: a chain of three (cnt = 2 in the middle); 6-32: a
    3 x 3 x 3 block at spacing 1.6 r; 33, 34 coincident with 35 overlapping both (the partner NEXT in memory); 0 and 37 coincident with 36
    overlapping both (the partner far away, the third particle between them).  A coincident pair alone would part to exactly 2 r, on the
    threshold of `pair`: with a third particle cnt = 2, they part by r and go on overlapping.  Every substep a placement of its own (seeded
    jitter and velocities): a pile left to itself relaxes to touching, d = 2 r +- rounding, which no band can call determined"""
    cup = W.dk.view(W.state[None])['free'][0, 0, :3].astype(np.float64)
    base = cup + [0, 0, 0.6]
    slots = np.zeros((38, 3))
    slots[1], slots[2] = [0.1, 0, 0], [0.1 + 1.5 * R, 0, 0]
    slots[3], slots[4], slots[5] = [0.2, 0, 0], [0.2 + 1.7 * R, 0, 0.001], [0.2 + 3.4 * R, 0, 0]
    slots[6:33] = [[0.3 + 1.6 * R * i, 1.6 * R * j, 1.6 * R * k] for i in range(3) for j in range(3) for k in range(3)]
    slots[33] = slots[34] = [0.0, 0.1, 0]
    slots[35] = [1.2 * R, 0.1, 0.0005]
    slots[0] = slots[37] = [0.1, 0.1, 0]
    slots[36] = [0.1, 0.1 + 1.3 * R, -0.0005]
    rec = _scene(np.zeros((38, 3)), [])

    def place(k):
        rs = np.random.RandomState(500 + k)
        x = (base + slots + rs.uniform(-2e-4, 2e-4, slots.shape)).astype(np.float32)
        v = rs.uniform(-0.05, 0.05, slots.shape).astype(np.float32)
        for a, b in ((33, 34), (0, 37)):
            x[b], v[b] = x[a], v[a]
        return x, v

    def cond(rows):
        c = np.max([r['M']['cnt'] for r in rows], axis=0)
        ok = c[1] == 1 and c[2] == 1 and c[4] == 2 and c[6:33].max() >= 6 and all(r['M']['eps'][[33, 34, 0, 37]].max() < 1.2e-7 for r in rows)
        return [] if ok else ['counts %s' % c]
    return rec, [W.state], place, 16, False, cond


def ww_cup_rest(W, water):
    """the real cup (68 convex pieces, first in the drinking scene's own shape list of 179) in the settled state with the 64 particles.  A
    pile AT REST sits on every threshold at once (particles on the planes they were projected onto, neighbours at 2 r +- rounding), so the
    inputs are the settled pile shaken: every substep starts from the settled positions with a seeded jitter of 0.2 mm and seeded velocities
    of up to 0.3 m/s, which press the particles into the walls and into each other or take them off.  Determined substeps only are kept"""
    dk = W.dk
    ids = [s['collider'] for s in WC.shape_table(dk)]
    x0 = WC.tables(dk)['x0']
    rec = _scene(x0, ids, dict(KDF=4.0, PITER=3))

    def place(k):
        rs = np.random.RandomState(9000 + k)
        return (water[0] + rs.uniform(-2e-4, 2e-4, water[0].shape)).astype(np.float32), rs.uniform(-0.3, 0.3, water[0].shape).astype(np.float32)

    def cond(rows):
        return [] if min(len(r['hits']) for r in rows) >= 20 else ['few hits']
    return rec, [W.state], place, 1500, False, cond


def _shoulder_top(W):
    (a, b), rad = W.ends(W.person(SHOULDER_L))
    return a, b, rad


def ww_cap(W, variant):
    """a: the left shoulder capsule listed 14 times, eight particles resting along its top and two out of reach: every lane that touches fills
    its 12 slots with copies and drops the 13th and 14th.  b: 11 copies, then the right shoulder, then the head; particles in the notch in front
    of the neck where the three meet: the 12th slot holds the right shoulder, the head is the 13th candidate and is dropped (the particles go
    on into it).  kDF = 4: kDF x friction = 2, capped at 1 -- the copies of a touched shape are touched or not by rounding (d = 0 after the
    first), and only with the whole tangential velocity gone after the first does that leave the result alone"""
    c = W.person(SHOULDER_L)
    a, b, rad = _shoulder_top(W)
    if variant == 'a':
        ids = [c] * 14
        us = np.linspace(0.0, 1.0, 4)
        x = [a + u * (b - a) + np.array([0, dy, np.sqrt((rad + R - 1e-4) ** 2 - dy * dy)]) for u in us for dy in (-0.012, 0.012)]
        x += [a + [0, 0, rad + 0.05], a + [0.0, -0.3, 0.3]]
        x = np.array(x)
        v = np.zeros_like(x) + [0.02, 0.0, 0.0]
        rec = _scene(np.zeros((len(x), 3)), ids, dict(KDF=4.0, PITER=3))

        def cond(rows):
            ok = all((r['info']['ncand'][:8] == 12).all() and (r['info']['ncand'][8:] == 0).all() and len(r['hits']) == 8 for r in rows)
            return [] if ok else ['not every touching lane full']
        return rec, [W.state], lambda k: (x.astype(np.float32), v.astype(np.float32)), 14, True, cond
    ids = [c] * 11 + [W.person(SHOULDER_R), W.person(HEAD)]
    (ha, hb), hrad = W.ends(W.person(HEAD))
    (ra, rb), rrad = W.ends(W.person(SHOULDER_R))
    # the notch: on the head's cylinder in front (y < axis), at the height where both shoulders' inner ends are rad + R away
    yy = hrad + R
    inner_l, inner_r = (a if abs(a[0]) < abs(b[0]) else b), (ra if abs(ra[0]) < abs(rb[0]) else rb)
    zz = inner_l[2] + np.sqrt((rad + R) ** 2 - inner_l[0] ** 2 - yy ** 2)
    p = np.array([0.5 * (inner_l[0] + inner_r[0]), ha[1] - yy, zz])
    rec = _scene(np.zeros((5, 3)), ids, dict(KDF=4.0, PITER=3))

    def place(k):
        off = np.array([[0, 0, 0], [0.004, 0, 0.001], [-0.004, 0, 0.001], [0.0, 0.0, 0.012], [0, -0.3, 0.3]]) + [0, -0.0005 - 0.0001 * k, 0.0005]
        v = np.zeros((5, 3)) + [0.0, 0.4, -0.3]
        return (p + off).astype(np.float32), v.astype(np.float32)

    def cond(rows):
        ok = all((r['info']['ncand'][:3] == 12).all() and all(s[-1] == 11 for s in r['info']['slots'][:3]) and any((i, 11) in r['hits'] for i in range(3)) for r in rows)
        return [] if ok else ['the 12th slot does not hold the right shoulder, touched']
    return rec, [W.state], place, 14, False, cond


def ww_chunks(W):
    """NS = 192: the shapes touched sit at list indices 0, 63, 64, 127, 128 and 191 (the ends of the three 64-shape rounds in which the
    kernel builds its list), every other entry a collider out of reach"""
    dk = W.dk
    touched = [W.person(b) for b in (THIGH_L, THIGH_R, FOREARM_L, FOREARM_R, HAND_L, HAND_R)]
    at = [0, 63, 64, 127, 128, 191]
    others = [c for c in range(dk.h['NCOLL']) if c not in touched and c not in range(*W.r['human_male']) and c not in range(*W.r['human_female'])]
    ids = [others[k % len(others)] for k in range(192)]
    for k, c in zip(at, touched):
        ids[k] = c
    x, v = [], []
    for c in touched:
        ends, rad = W.ends(c)
        if len(ends) == 2:
            for u in (0.35, 0.6):
                p, d, ax = W.on_capsule(c, u, [0, 0, 1], 2e-4)
                x.append(p); v.append(-0.3 * d + 0.1 * ax)
        else:
            for dx in (-0.01, 0.012):
                d = np.array([dx, 0.0, np.sqrt(1 - (dx / (rad + R)) ** 2) * (rad + R)]) / (rad + R)
                x.append(ends[0] + d * (rad + R + 2e-4)); v.append(-0.3 * d)
    x, v = np.array(x), np.array(v)
    rec = _scene(np.zeros((len(x), 3)), ids)
    rec['touched_at'] = at

    def cond(rows):
        want = {(2 * j + e, at[j]) for j in range(6) for e in range(2)}
        return [] if all(r['hits'] == want for r in rows) else ['hits %s' % sorted(rows[0]['hits'])]
    return rec, [W.state], lambda k: (x.astype(np.float32), v.astype(np.float32)), 14, True, cond


def ww_planes(W):
    """hulls that keep 5, 7 and 8 of their face planes (padded to 8, 8 and 8 with the last kept one) and the hull with the most planes in the
    blob (a finger of the gripper: 122 planes padded to 124), a particle of 2 mm radius dropped onto the FIRST, a MIDDLE and the LAST real
    plane of each: an off-by-one in the four-plane prefetch loses the last plane, a padded duplicate that wins changes nothing but its index"""
    from assistive_gym_amd.model.cloth import hull_planes
    dk = W.dk
    rr = 0.002
    big = [c for c in range(dk.h['NCOLL']) if len(dk.collider(c)['verts']) > 2]
    counts = {c: len(hull_planes(dk.collider(c)['verts'])) for c in big}
    finger = max(counts, key=lambda c: (counts[c], -c))
    wheel = [c for c in range(*W.r['wheelchair']) if counts[c] >= 20][:3]
    ids, keep = wheel + [finger], {0: 5, 1: 7, 2: 8}
    x, v, want = [], [], []
    for k, c in enumerate(ids):
        col = dk.collider(c)
        P = hull_planes(col['verts'])
        n = keep.get(k, counts[c])
        p, Rm = W.frames[col['body']]
        def spot(f):
            on = np.abs(col['verts'] @ P[f, :3] - P[f, 3]) < 1e-6
            cen = col['verts'][on].mean(0) + P[f, :3] * (col['radius'] + rr + 1e-4)      # the particle's centre, 0.1 mm of air under it
            tt = P[:n, :3] @ cen - P[:n, 3]
            oth = np.abs(P[:n] - P[f]).max(1) > WC.SAME_PLANE
            return cen, ((tt[f] - tt[:n][oth]) / np.maximum(np.linalg.norm(P[:n][oth, :3] - P[f, :3], axis=1), WC.PLANE_TURN)).min()
        mid = next(f for f in list(range(n // 2, n - 1)) + list(range(n // 2, 0, -1)) if spot(f)[1] > 1e-4)      # a middle plane that leads clearly over its centre
        for f in (0, mid, n - 1):
            cen = spot(f)[0]
            x.append(p + Rm @ cen); v.append(Rm @ (-0.2 * P[f, :3])); want.append((k, f))
    x, v = np.array(x), np.array(v)
    rec = _scene(np.zeros((len(x), 3)), ids, keep_planes=keep, radius=rr)
    rec['faces'] = want
    rec['moving'] = True

    def place(k):
        return (x + np.array(v) * 0.0003 * k).astype(np.float32), v.astype(np.float32)      # a little nearer every time

    def cond(rows):
        msg = []
        for r in rows:
            for i, (k, f) in enumerate(want):
                if (i, k) not in r['hits'] or r['info']['faces'][i][r['info']['slots'][i].index(k)] != f:
                    msg.append('particle %d not on plane %d of hull %d' % (i, f, k))
        return msg[:3]
    return rec, [W.state], place, 14, False, cond


def ww_cores(W):
    """capsule and sphere cores: particles dropped onto the left forearm along its length with a velocity ACROSS it (the tangent plane turns with
    the particle: taken where the substep starts), around the left hand's sphere, onto the top end of the head's capsule and the knee end of
    the left thigh's exactly along their axes (t clamped at 1 and at 0), one fast one that starts beyond 2 r and reaches the forearm only
    through its |v| dt, and two that touch nothing"""
    fa, hand, head, thigh = W.person(FOREARM_L), W.person(HAND_L), W.person(HEAD), W.person(THIGH_L)
    ids = [fa, hand, head, thigh]
    x, v = [], []
    for u, ang in ((0.45, 0.0), (0.55, 0.5), (0.65, -0.6), (0.75, 1.0)):
        p, d, ax = W.on_capsule(fa, u, [np.sin(ang), 0, np.cos(ang)], 2e-4)
        x.append(p); v.append(-0.3 * d + 0.8 * np.cross(ax, d))
    (hc,), hrad = W.ends(hand)
    for d in ([0, 0, 1.0], [0.6, 0, 0.8], [0, -0.8, 0.6]):
        d = np.array(d)
        x.append(hc + d * (hrad + R + 2e-4)); v.append(-0.3 * d)
    (a, b), rad = W.ends(head)
    ax = (b - a) / np.linalg.norm(b - a)
    x.append(b + ax * (rad + R + 2e-4)); v.append(-0.3 * ax)
    (a, b), rad = W.ends(thigh)
    ax = (b - a) / np.linalg.norm(b - a)
    x.append(a - ax * (rad + R + 2e-4)); v.append(0.3 * ax)
    p, d, ax = W.on_capsule(fa, 0.3, [0, 0, 1], 0.012)
    x.append(p); v.append(-3.0 * d)
    p, d, ax = W.on_capsule(fa, 0.2, [0, 0, 1], 0.004)
    x.append(p); v.append(1.0 * d)                                      # in reach, moving away: a candidate that is never touched
    x.append(np.array(x[0]) + [0, -0.3, 0.4]); v.append(np.zeros(3))
    x, v = np.array(x), np.array(v)
    rec = _scene(np.zeros((len(x), 3)), ids)
    rec['moving'] = True

    def place(k):
        return (x + v * 0.0002 * k).astype(np.float32), v.astype(np.float32)

    def cond(rows):
        want = {(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 1), (6, 1), (7, 2), (8, 3), (9, 0)}
        return [] if all(r['hits'] == want and r['info']['ncand'][10] == 1 for r in rows) else ['hits %s' % sorted(rows[0]['hits'])]
    return rec, [W.state], place, 14, False, cond


def ww_gender(W):
    """both genders' copies of the left thigh and the left forearm are listed (the male one first for the thigh, second for the forearm), one
    state record per gender: particles dropped into the gap between the two copies' radii touch only the copy of the record's gender"""
    ids = [W.person(THIGH_L, 0), W.person(THIGH_L, 1), W.person(FOREARM_L, 1), W.person(FOREARM_L, 0)]
    x, v = [], []
    for c, us in ((ids[0], (0.3, 0.5, 0.7)), (ids[3], (0.4, 0.6))):
        for u in us:
            p, d, ax = W.on_capsule(c, u, [0, 0, 1], 2e-4)               # just above the larger (male) copy
            x.append(p); v.append(-1.6 * d)                               # 8 mm in the substep: past the gap to the smaller (female) copy
    x, v = np.array(x), np.array(v)
    states = []
    for g in (0, 1):
        s = W.state.copy()
        W.dk.view(s[None])['gender'][0] = g
        states.append(s)
    rec = _scene(np.zeros((len(x), 3)), ids)

    def place(k):
        return (x + v * 0.00005 * (k // 2)).astype(np.float32), v.astype(np.float32)

    def cond(rows):
        msg = []
        for r in rows:
            g = int(W.dk.view(r['state'][None])['gender'][0])
            want = {(i, (0, 1)[g]) for i in range(3)} | {(i, (3, 2)[g]) for i in (3, 4)}
            if r['hits'] != want:
                msg.append('gender %d hits %s' % (g, sorted(r['hits'])))
        return msg[:2]
    return rec, states, place, 24, False, cond      # placement k uses states[k % 2]


def ww_friction(W):
    """kDF = 3 and the colliders' friction patched to 0.1 (left thigh: kDF x friction = 0.3) and 1.0 (right thigh: 3.0, capped at 1):
    particles sliding along and across each"""
    cl, cr = W.person(THIGH_L), W.person(THIGH_R)
    x, v = [], []
    for c in (cl, cr):
        for u, ang in ((0.3, 0.0), (0.45, 0.3), (0.6, -0.4)):
            p, d, ax = W.on_capsule(c, u, [np.sin(ang), 0, np.cos(ang)], -1e-4)
            x.append(p); v.append(0.4 * ax + 0.2 * np.cross(ax, d))
    x, v = np.array(x), np.array(v)
    rec = _scene(np.zeros((len(x), 3)), [cl, cr], dict(KDF=3.0, KDP=0.01), friction={cl: 0.1, cr: 1.0})

    def cond(rows):
        want = {(i, 0) for i in range(3)} | {(i, 1) for i in range(3, 6)}
        return [] if all(r['hits'] == want for r in rows) else ['hits %s' % sorted(rows[0]['hits'])]
    return rec, [W.state], lambda k: (x.astype(np.float32), v.astype(np.float32)), 14, True, cond


def ww_hit_last(W):
    """a LAUNCH: one settle(1) of the ordinary four-substep blob from a state with joint velocities (the cup moves 1e-3 m per substep).
    Particles 0-3 rest on the thighs (touched in every substep: flag 1), 4 and 5 graze the top of the left thigh at 4 m/s across it (touched in
    the first substeps, gone by the last: flag 0), 6-9 stand on the bottom of the moving cup (the free body, read from the trace slot of
    each substep), 10 falls free"""
    dk = W.dk
    ids = [s['collider'] for s in WC.shape_table(dk)]
    state = W.state.copy()
    v_ = dk.view(state[None])
    v_['qd'][0, :7] = [0.3, -0.3, 0.3, 0.2, -0.2, 0.2, 0.1]
    x, v = [], []
    for c, u in ((W.person(THIGH_L), 0.4), (W.person(THIGH_L), 0.6), (W.person(THIGH_R), 0.4), (W.person(THIGH_R), 0.6)):
        p, d, ax = W.on_capsule(c, u, [0, 0, 1], -1e-4)
        x.append(p); v.append(np.zeros(3))
    for u in (0.25, 0.75):
        p, d, ax = W.on_capsule(W.person(THIGH_L), u, [0, 0, 1], 1e-4)
        x.append(p - 0.012 * np.cross(ax, d)); v.append(4.0 * np.cross(ax, d) - 0.2 * d)
    return dict(state=state, ids=ids, x=x, v=v)


SCENES = ['ww_free_1', 'ww_free_2', 'ww_free_63', 'ww_free_64', 'ww_pile', 'ww_cup_rest', 'ww_cap_a', 'ww_cap_b', 'ww_chunks', 'ww_planes', 'ww_cores', 'ww_gender',
          'ww_friction', 'ww_hit_last']


def build(W, water, name):
    if name.startswith('ww_free'):
        return ww_free(W, int(name.split('_')[2]))
    if name.startswith('ww_cap'):
        return ww_cap(W, name[-1])
    if name == 'ww_cup_rest':
        return ww_cup_rest(W, water)
    return globals()[name](W)


def hit_last_scene(W):
    """(see ww_hit_last) the cup's particles stand on its bottom (6.5 mm above the cup's origin along its axis, the mesh y axis), seeded places
    within 15 mm of the axis, apart from each other; launches are tried until enough are determined (the bottom and the wall are made of many
    pieces: a particle that comes to rest on a seam is on the threshold of the neighbouring piece for the rest of the launch)"""
    h = ww_hit_last(W)
    tp, tR = W.frames[L.BODY_FREE0]
    x0 = np.array(h['x'] + [np.zeros(3)] * 4 + [np.array(h['x'][0]) + [0, -0.3, 0.5]])
    v0 = np.array(h['v'] + [np.zeros(3)] * 4 + [np.array([0.1, 0.0, 0.0])])
    rec = _scene(np.zeros((len(x0), 3)), h['ids'], nsub=4)
    rec['moving'] = True

    def place(k):
        rs = np.random.RandomState(700 + k)
        xx, vv = x0.copy(), v0.copy()
        xx[4:6, 0] += 0.0004 * (k % 10)         # the grazing particles a little further on every time
        rel = []
        while len(rel) < 4:
            c = rs.uniform(-0.015, 0.015, 2)
            if np.hypot(*c) < 0.015 and all(np.hypot(*(c - o)) > 0.0125 for o in rel):
                rel.append(c)
        xx[6:10] = [tp + tR @ np.array([c[0], 0.0065 + R + 3e-4, c[1]]) for c in rel]
        vv[6:10] = rs.uniform(-0.02, 0.02, (4, 3)) + [0, 0, -0.1]
        return xx.astype(np.float32), vv.astype(np.float32)
    return rec, [h['state']], place, 120, False, None


def run(dk, W, water, name, limit=None):
    from oracle_lib import Oracle
    launch = name == 'ww_hit_last'
    rec, states, place, n_try, evolve, cond = hit_last_scene(W) if launch else build(W, water, name)
    if limit:
        n_try = min(n_try, limit)
    blob = WC.case_blob(rec)
    o = Oracle(blob)
    t, shapes = WC.tables(blob), WC.shape_table(blob)
    moving = bool(rec.get('moving')) or name == 'ww_cup_rest'
    rows, x, v = [], None, None
    want = KEEP if name in ('ww_cup_rest', 'ww_hit_last') else None      # tried until enough are determined
    for k in range(n_try):
        state = states[k % len(states)]
        gender = int(dk.view(state[None])['gender'][0])
        if x is None or not evolve:
            x, v = place(k)
        if launch:
            trace, _ = WC.oracle_trace(blob, o, state, np.stack([x, v]), rec['nsub'])
            mov = [WC.moving_of_trace(trace, j) for j in range(rec['nsub'])]
            assert np.abs(np.diff(trace[:, blob.ndof, :3], axis=0)).max(1).min() >= 1e-4, 'the cup moves less than 1e-4 m between two trace slots'
        else:
            mov = [WC.moving_of_state(blob, o, state)]
        fr = lambda dtype, shift=0: [WC.body_frames(blob, state, m, dtype, shift) for m in mov]
        per = []
        xx, vv = x.astype(np.float64), v.astype(np.float64)
        for f in fr(np.float64):                 # substep by substep, for the per-substep hits of a launch
            xx, vv, hits, M, info = WC.substep(t, shapes, f, xx, vv, gender=gender)
            per.append((hits, M))
        x64, v64 = xx, vv
        Mall = {key: (np.maximum if key == 'cnt' else np.minimum).reduce([m[key] for _, m in per]) for key in per[0][1]}
        det = WC.determined(Mall)
        row = dict(sub=k, det=det, state=state, xin=x, vin=v, x=x64, v=v64, hits=hits, M=Mall, info=info, per=[h for h, _ in per], why=WC.undetermined_by(Mall), dev=np.full(4, np.inf))
        if det:
            dev = np.zeros(4)
            for shift in ((0, 1, -1) if moving else (0,)):
                x32, v32, h32, _, _ = WC.substeps(t, shapes, fr(np.float32, shift), x, v, gender=gender, dtype=np.float32)
                assert h32 == hits, (name, k, 'the float32 restatement found other hits in a determined substep')
                dev = np.maximum(dev, WC.deviation(x32, v32, x64, v64, info['here']))
            row['dev'] = dev
        rows.append(row)
        if evolve:
            x, v = x64.astype(np.float32), v64.astype(np.float32)
        if want and sum(r['det'] for r in rows) >= want:
            break
    return rec, rows, cond


def make_scene(dk, W, water, name, log=print, limit=None):
    rec, rows, cond = run(dk, W, water, name, limit)
    det = [r for r in rows if r['det']]
    msg = cond(det) if cond and det else []
    if name == 'ww_hit_last' and det:
        shapes = WC.shape_table(WC.case_blob(rec))
        for r in det:
            person = [{i for i, sh in h if shapes[sh]['human']} for h in r['per']]
            if not ({4, 5} <= person[0] | person[1] and not {4, 5} & person[3] and {0, 1, 2, 3} <= person[3] and {(i, s) for i, s in r['hits'] if i in (6, 7, 8, 9)}):
                msg.append('launch %d: person hits per substep %s' % (r['sub'], person))
    if len(det) < 10:
        msg.append('%d determined substeps of %d (undetermined by band: %s)' % (len(det), len(rows), {k: sum(k in r['why'] for r in rows) for k in WC.BAND}))
    if msg and limit is None:
        raise RuntimeError(name + ': ' + '; '.join(msg[:4]))
    keep = sorted(det[:KEEP] + [r for r in rows if not r['det']][:0 if name == 'ww_cup_rest' else KEEP_OTHER], key=lambda r: r['sub'])      # (the cup: determined substeps only)
    hit = np.array([(k, i, s) for k, r in enumerate(keep) for (i, s) in sorted(r['hits'])], dtype=np.int16).reshape(-1, 3)
    mask = np.array([r['det'] for r in rows])
    kdet = np.array([r['det'] for r in keep])
    dev = np.array([np.where(np.isfinite(r['dev']), r['dev'], 0.0) for r in keep])
    rec.update(determined=int(mask.sum()), tried=len(rows), hits_compared=int(sum(len(r['hits']) for r in det[:KEEP])))
    log('%s: %d of %d substeps determined, %d stored; %d hits; float32 deviation x %.2e v %.2e (parked: x %.2e v %.2e)'
        % (name, mask.sum(), len(rows), len(keep), rec['hits_compared'], *(dev[kdet].max(0) if kdet.any() else np.zeros(4))))
    xin = np.array([r['xin'] for r in keep])
    return {name + '/recipe': np.array(json.dumps(rec)), name + '/mask': mask, name + '/sub': np.array([r['sub'] for r in keep], dtype=np.int16), name + '/det': kdet,
            name + '/state': np.array([r['state'] for r in keep]), name + '/xin': xin, name + '/vin': np.array([r['vin'] for r in keep]),
            name + '/dx': (np.array([r['x'] for r in keep]) - xin.astype(np.float64)).astype(np.float32), name + '/v': np.array([r['v'] for r in keep]).astype(np.float32),
            name + '/hit': hit, name + '/dev': dev}


def make(names=None, log=print, limit=None):
    dk = load()
    state, water = settled(dk)
    W = World(dk, state)
    out = {}
    for name in (names or SCENES):
        out.update(make_scene(dk, W, water, name, log, limit))
    return out


def main():
    names = sys.argv[1:] or None
    out = make(names)
    if names:
        old = dict(np.load(OUT)) if os.path.exists(OUT) else {}
        old.update(out)
        out = old
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
