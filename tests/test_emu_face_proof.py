"""Face pairs of the build kernel's narrowphase (csrc/agx_collide.h, AGX_FACE) on the CPU wave emulator.  A collider resting on a static world box
-- in the feeding scene the bowl's pieces on the table top -- takes 1 + AGX_FACE_EXTRA worklist entries; the default build computes their vertex
contacts with eight vertices per loop round and one zmin per pair, and entry 0 skips GJK where the pair is PROVEN to be a face contact (footprint
inside the box's, core gap inside its guard band).  -DAGX_FACE_PLAIN runs GJK for every pair and the one-vertex loops, as the kernel did before.
Both must end every env step in the SAME BITS: observation, reward, done, info, the state record and the debug record of the first substep (its
contact records included; the cycle counters are not results).
The -DAGX_EMU_TRACE_GJK twins show which path ran: a traced row is one gjk_distance lane, a proven pair leaves none.  A face pair's row is one
with a box partner and a hull of at least two vertices; its core distance and its limit (+ radii + GJK_FAR_MARGIN) are recorded in micrometres."""
import ctypes as C
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import emu_lib
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.host.reset import make_states

emu_lib.derive('feeding_face_plain', 'feeding', ['-DAGX_FACE_PLAIN'])
emu_lib.derive('feeding_trace_face_plain', 'feeding', ['-DAGX_EMU_TRACE_GJK', '-DAGX_FACE_PLAIN'])
NEW, PLAIN, NEW_T, PLAIN_T = 'feeding', 'feeding_face_plain', 'feeding_trace', 'feeding_trace_face_plain'
N_STATES, N_STEPS = 6, 30
BOWL = 1                       # free body 1 of the feeding scene: the bowl (about 100 hull pieces), resting on the table top
FAR_MARGIN_UM = 100            # GJK_FAR_MARGIN: the traced limit is lim + radii + this
GUARD_UM, GUARD_LIM_UM = 100, 10      # FACE_PROOF_GUARD, FACE_PROOF_GUARD_LIM (csrc/agx_collide.h)
EDGE_UM = 2                    # the trace truncates to whole micrometres: rows this close to a guard are not asked about


@pytest.fixture(scope='module')
def settled(blob, oracle):
    """settled start states: the bowl rests on the table, the food on the spoon (the pool's 25 settle substeps)"""
    st, _ = make_states(blob, N_STATES, seed=4242)
    for i in range(N_STATES):
        oracle.settle(st[i], 25)
    return st


@pytest.fixture(scope='module')
def emus(blob):
    """12 solver sweeps instead of 50, as tests/test_emu_parity.py (a step emulates in a third of the time); `one`: one substep per env step, so
    that the narrowphase of a step sees exactly the pose of the state record"""
    b12 = blob.set_param('NITER', 12)
    b1 = b12.set_param('FRAME_SKIP', 1)
    return dict(step={k: emu_lib.Emu(b12, kind=k) for k in (NEW, PLAIN, NEW_T, PLAIN_T)}, one={k: emu_lib.Emu(b1, kind=k) for k in (NEW_T, PLAIN_T)})


def _words(e, out, s):
    obs, rew, done, info, dbg = out
    r = dict(obs=obs.view(np.uint32), reward=np.float32(rew).view(np.uint32), done=np.uint8(done), info=info.view(np.uint32), state=s.view(np.uint32).copy())
    if dbg is not None:
        # the debug record of the first substep: its head words (contact and row counts), the contact records, the inverse mass matrix and the
        # accelerations.  (Not the copy of the scratch record's row headers and impulses: beyond the rows of this substep it holds what earlier
        # steps of the same emulator library left there; and not the cycle counters.)
        d = dbg.view(np.uint32)
        r['debug'] = np.concatenate([d[:16], d[e.DBG_CON:e.DBG_CON + 16 * int(dbg[0])], d[e.DBG_MINV:e.DBG_HDR], d[e.DBG_QDD:]])
    return r


def _step(e, state, action):
    """one env step from a copy of `state` without warm-start memory -> every output, the new record and the first substep's debug record, as raw words"""
    s = state.copy()
    e.forget_warm()
    return _words(e, e.step(s, action, debug=True), s)


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), '%s: %s differs between the default build and -DAGX_FACE_PLAIN' % (what, k)


def _traced(e, state, action):
    """(face-pair rows (|A|, iterations, stopped by the bound, core distance um, limit um) of one env step on a traced build, its outputs)"""
    tr = (C.c_int * (1 << 22)).in_dll(e.L, 'g_gjk_trace'); n = C.c_int.in_dll(e.L, 'g_gjk_n')
    n.value = 0
    out = _step(e, state, action)
    t = np.frombuffer(tr, dtype=np.int32, count=n.value).reshape(-1, 9)
    f = t[(t[:, 5] == 1) & (t[:, 3] >= 2)]
    return [tuple(int(x) for x in r[[3, 2, 6, 7, 8]]) for r in f], out


def _margin(row):
    """limit minus separation of a traced face row, um"""
    return row[4] - FAR_MARGIN_UM - row[3]


def _paths(emus, state, what):
    """one substep of `state` on both traced builds: the same bits; -> (rows of the plain build, the rows among them that the default build did
    not run: the proven pairs).  Every proven row lies inside both guards; that every row inside both guards is proven is for the caller to ask
    (it takes the footprint as well)."""
    a = np.zeros(emus['one'][NEW_T].blob.act_dim, dtype=np.float32)
    rn, on = _traced(emus['one'][NEW_T], state, a)
    rp, op = _traced(emus['one'][PLAIN_T], state, a)
    _same(on, op, what + ' (one substep, traced builds)')
    left = Counter(rn) - Counter(rp)
    assert not left, '%s: the default build ran GJK for face pairs the plain build does not have: %s' % (what, left)
    proven = Counter(rp) - Counter(rn)
    for r in proven:
        assert r[3] >= GUARD_UM - 1 and _margin(r) >= GUARD_LIM_UM - 1 and r[2] == 0, '%s: a pair outside the guards was skipped: %s' % (what, (r,))
    return rp, proven


def _inside_guards(r):
    return r[3] >= GUARD_UM + EDGE_UM and _margin(r) >= GUARD_LIM_UM + EDGE_UM


def _full_step_same(blob, emus, state, what):
    a = np.zeros(blob.act_dim, dtype=np.float32)
    ref = _step(emus['step'][NEW], state, a)
    _same(ref, _step(emus['step'][PLAIN], state, a), what)
    return ref


def _bowl(blob, state, dpos=(0.0, 0.0, 0.0), quat=None, pos=None):
    """a copy of `state` with the bowl at rest, moved by dpos (or at pos) and, with quat (x, y, z, w), turned by it about its own origin"""
    s = state.copy()
    r = blob.view(s)['free'][0, BOWL]
    r[7:13] = 0.0                  # at rest: the limit of its pairs is then slack + 1e-5 whatever the placement
    r[:3] = (r[:3].astype(np.float64) + np.array(dpos)).astype(np.float32) if pos is None else pos
    if quat is not None:
        x1, y1, z1, w1 = quat; x2, y2, z2, w2 = r[3:7].astype(np.float64)
        r[3:7] = (w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2)
    return s


@pytest.fixture(scope='module')
def rest(blob, emus, settled):
    """the bowl at rest where it settled, and the face rows of that pose"""
    s = _bowl(blob, settled[0])
    rows, proven = _paths(emus, s, 'rest')
    return s, rows, proven


def test_bowl_at_rest_is_proven(blob, emus, rest):
    """every piece of the resting bowl that GJK would find in contact, footprint well inside the table's, is proven: no trace row"""
    s, rows, proven = rest
    hits = [r for r in rows if _margin(r) > 0]
    assert len(hits) >= 6, 'fixture: the resting bowl must have face pairs (the plain build shows %d)' % len(hits)
    want = Counter(r for r in rows if _inside_guards(r))
    assert sum(want.values()) >= 6 and not (want - proven), 'pairs inside both guards that ran GJK: %s' % (want - proven)
    assert sum(proven.values()) >= 0.9 * len(hits)
    ref = _full_step_same(blob, emus, s, 'rest')
    # the traced builds compute what the plain ones do
    a = np.zeros(blob.act_dim, dtype=np.float32)
    _same({k: v for k, v in ref.items()}, _traced(emus['step'][NEW_T], s, a)[1], 'rest (traced against untraced)')


@pytest.mark.parametrize('case', ['lim_in', 'lim_out', 'low_shell'])
def test_guard_shells_take_gjk(blob, emus, rest, case):
    """the bowl lifted (lowered) so that one of its pieces sits 5 um inside its limit, 5 um outside it, or with its core 50 um above the table's:
    inside the shell of FACE_PROOF_GUARD_LIM / FACE_PROOF_GUARD that piece runs GJK in both builds, the pieces clear of the guards stay proven.
    (Around the limit the bowl is first turned by 2 degrees: the broadphase drops a level piece at limit - 11 um, a turned piece's box is looser.)"""
    s0, rows, _ = rest
    a = np.zeros(blob.act_dim, dtype=np.float32)
    if case == 'low_shell':
        base = s0
        offsets = [-(min(r[3] for r in rows if _margin(r) > 0) - 50)]
        shell = lambda r: 1 + EDGE_UM <= r[3] <= GUARD_UM - EDGE_UM
    else:
        h = np.radians(1.0)
        base = _bowl(blob, s0, quat=(np.sin(h), 0.0, 0.0, np.cos(h)))
        margins = sorted(_margin(r) for r in _traced(emus['one'][PLAIN_T], base, a)[0] if r[2] == 0 and r[3] > GUARD_UM)
        offsets = [m - 5 if case == 'lim_in' else m + 5 for m in margins]
        shell = (lambda r: EDGE_UM <= _margin(r) <= GUARD_LIM_UM - EDGE_UM) if case == 'lim_in' else (lambda r: -GUARD_LIM_UM + EDGE_UM <= _margin(r) <= -EDGE_UM)
    for dz_um in offsets:          # the first offset that leaves a piece in the shell (the broadphase may drop the piece it was computed for)
        s = _bowl(blob, base, dpos=(0.0, 0.0, dz_um * 1e-6))
        if any(shell(r) for r in _traced(emus['one'][PLAIN_T], s, a)[0]):
            break
    rp, proven = _paths(emus, s, case)
    in_shell = [r for r in rp if shell(r)]
    assert in_shell, '%s: no piece in the shell; rows %s' % (case, sorted(rp))
    assert not any(r in proven for r in in_shell)
    want = Counter(r for r in rp if _inside_guards(r))
    assert not (want - proven), '%s: pairs inside both guards that ran GJK: %s' % (case, want - proven)
    _full_step_same(blob, emus, s, case)


def test_overhanging_pieces_take_gjk(blob, emus, rest):
    """the bowl shifted to the table's edge (y = -0.5): the pieces over the edge, and those whose box comes within the guard of it, run GJK"""
    s0, rows, proven0 = rest
    y = float(blob.view(s0.copy())['free'][0, BOWL, 1])
    s = _bowl(blob, s0, dpos=(0.0, -0.5 - y, 0.0))
    rp, proven = _paths(emus, s, 'overhang')
    assert 0 < sum(proven.values()) < sum(proven0.values())
    assert sum((Counter(r for r in rp if _inside_guards(r)) - proven).values()) > 0         # inside the guards in z, yet not proven: the footprint
    _full_step_same(blob, emus, s, 'overhang')


def test_tilted_bowl(blob, emus, rest):
    """the bowl turned by 20 degrees about x"""
    s0, rows, _ = rest
    h = np.radians(10.0)
    s = _bowl(blob, s0, quat=(np.sin(h), 0.0, 0.0, np.cos(h)))
    rp, proven = _paths(emus, s, 'tilted')
    assert len(rp) > sum(proven.values()), 'the tilted bowl must leave pairs to GJK'
    _full_step_same(blob, emus, s, 'tilted')


def test_bowl_pushed_into_the_table(blob, emus, rest):
    """2 mm down: the core of the lowest piece (1 mm above the table's at rest) overlaps it; that piece runs GJK in both builds"""
    s0, rows, _ = rest
    low = min((r for r in rows if _margin(r) > 0), key=lambda r: r[3])
    assert low[3] < 1900, 'fixture: a piece whose core is less than 2 mm above the table expected; rows %s' % sorted(rows)
    s = _bowl(blob, s0, dpos=(0.0, 0.0, -2e-3))
    rp, proven = _paths(emus, s, 'pushed')
    mine = [r for r in rp if r[0] == low[0]]          # by its hull size
    assert mine and not any(r in proven for r in mine)
    assert sum(proven.values()) > 0                   # the pieces higher up are still 3 mm clear
    _full_step_same(blob, emus, s, 'pushed')


def test_nan_pose_proves_nothing(blob, emus, rest):
    s0, _, _ = rest
    s = _bowl(blob, s0, pos=np.float32(np.nan))
    rp, proven = _paths(emus, s, 'NaN pose')
    assert not proven
    _full_step_same(blob, emus, s, 'NaN pose')


def test_rollouts_bit_identical_and_covered(blob, emus, settled):
    """6 settled states x 30 random-action steps, every third action three times as large: the same bits after every step, debug record included;
    the traced twins step alongside (the same bits again) and count the face pairs: the plain build shows them (about 8 per substep), and at
    least 90 % of them are proven in the default build"""
    rng = np.random.RandomState(13)
    kinds = (NEW, PLAIN, NEW_T, PLAIN_T)
    E = emus['step']
    tr = {k: ((C.c_int * (1 << 22)).in_dll(E[k].L, 'g_gjk_trace'), C.c_int.in_dll(E[k].L, 'g_gjk_n')) for k in (NEW_T, PLAIN_T)}
    rows = {NEW_T: 0, PLAIN_T: 0}
    pool = ThreadPoolExecutor(4)                  # four libraries with their own emulator state: they step side by side
    for i in range(N_STATES):
        s = {k: settled[i].copy() for k in kinds}
        for k in kinds:
            E[k].forget_warm()
        for j in range(N_STEPS):
            a = (rng.uniform(-1, 1, blob.act_dim) * (3.0 if j % 3 == 2 else 1.0)).astype(np.float32)
            for k in tr:
                tr[k][1].value = 0
            fut = {k: pool.submit(E[k].step, s[k], a, True) for k in kinds}
            out = {k: _words(E[k], fut[k].result(), s[k]) for k in kinds}
            for k in kinds[1:]:
                _same(out[NEW], out[k], 'state %d step %d (%s)' % (i, j, k))
            for k in tr:
                t = np.frombuffer(tr[k][0], dtype=np.int32, count=tr[k][1].value).reshape(-1, 9)
                rows[k] += int(((t[:, 5] == 1) & (t[:, 3] >= 2)).sum())
    pool.shutdown()
    substeps = N_STATES * N_STEPS * int(blob.param('FRAME_SKIP'))
    print('face pairs per substep: plain build %.2f, default build %.2f left to GJK' % (rows[PLAIN_T] / substeps, rows[NEW_T] / substeps))
    assert rows[PLAIN_T] >= 6 * substeps, 'the plain build must show the face pairs: %.2f per substep' % (rows[PLAIN_T] / substeps)
    assert rows[PLAIN_T] - rows[NEW_T] >= 0.9 * rows[PLAIN_T], 'proven: %d of %d face pairs' % (rows[PLAIN_T] - rows[NEW_T], rows[PLAIN_T])


# the other task / robot models of the bit comparisons of csrc/agx_gjk.h (profiles/r06/r06w_*), and a robot that stands on the ground plane
OTHERS = [('bed_bathing_sawyer', 'reset_bed', False), ('scratch_itch_pr2', 'reset_scratch', True), ('scratch_itch_jaco', 'reset_scratch', False),
          ('arm_manipulation_sawyer', 'reset_arm', False), ('dressing_baxter', 'reset_dressing', False), ('drinking_jaco', 'reset_drinking', False),
          ('feeding_sawyer', 'reset', False), ('feeding_panda', 'reset', False), ('feeding_baxter', 'reset', False), ('drinking_pr2', 'reset_drinking', False),
          ('scratch_itch_sawyer', 'reset_scratch', False), ('arm_manipulation_sawyer', 'reset_arm', True), ('feeding_stretch', 'reset', False)]


@pytest.mark.parametrize('name, module, coop', OTHERS, ids=['%s%s' % (n, '_human' if c else '') for n, _, c in OTHERS])
def test_other_models_bit_identical(name, module, coop):
    """one reset state, three random-action steps (the rigid scene of the dressing models, the water of the drinking ones included)"""
    import importlib
    b = ModelBlob.load(name)
    b = (b.coop() if coop else b).set_param('NITER', 12)
    made = importlib.import_module('assistive_gym_amd.host.' + module).make_states(b, 1, seed=7001)
    new = emu_lib.Emu(b)
    key = [k for k, v in emu_lib._LIBS.items() if v is new.L][0]
    emu_lib.derive('face_plain_%s' % key, key, ['-DAGX_FACE_PLAIN'])
    old = emu_lib.Emu(b, kind='face_plain_%s' % key)
    water = module == 'reset_drinking'
    s = [made[0][0].copy(), made[0][0].copy()]
    w = [np.ascontiguousarray(made[1][0]).copy(), np.ascontiguousarray(made[1][0]).copy()] if water else None
    new.forget_warm(); old.forget_warm()
    rng = np.random.RandomState(3)
    for j in range(3):
        a = rng.uniform(-1, 1, b.act_dim).astype(np.float32)
        if water:
            o = [e.step_water(s[q], w[q], a) for q, e in enumerate((new, old))]
            assert np.array_equal(w[0].view(np.uint32), w[1].view(np.uint32)), (name, j, 'water')
        else:
            o = [e.step(s[q], a) for q, e in enumerate((new, old))]
        assert np.array_equal(s[0].view(np.uint32), s[1].view(np.uint32)), (name, j, 'state record')
        assert np.array_equal(o[0][0].view(np.uint32), o[1][0].view(np.uint32)) and np.float32(o[0][1]).view(np.uint32) == np.float32(o[1][1]).view(np.uint32), (name, j, 'observation / reward')
        assert o[0][2] == o[1][2] and np.array_equal(o[0][3].view(np.uint32), o[1][3].view(np.uint32)), (name, j, 'done / info')
