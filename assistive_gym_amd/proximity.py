"""Batched closest-point queries between sets of colliders of a vec env (or a bare Stepper), answered on the device
(csrc/agx_proximity.hip through agx_proximity_set / agx_proximity, include/agx.h).

The reference reads distances between bodies through Agent.get_closest_points(agentB, distance, linkA, linkB) (assistive_gym/envs/agents/
agent.py:118-130), e.g. -min(tool.get_closest_points(human, distance=5.0)[-1]) in bed_bathing.py:23.  PyBullet answers per collision shape of
its own bodies; here a query names colliders of the model blob (spheres, capsules and convex hulls with a margin: what the stepper collides),
and every (environment, collider pair) is one closest-point computation of the stepper's own narrowphase.

  colliders(blob, tag, links)      collider indices by tag name, optionally by PyBullet link index
  ProximityQuery(env, queries)     .closest() every pair's record, .nearest() the nearest record of every query, per environment"""
import numpy as np

from .model import compiler as L

TAGS = {k.lower(): v for k, v in L.TAG.items()}      # 'robot', 'tool', 'human', 'food', 'bowl', 'table', 'plane', 'wheelchair', 'bed'
RECORD_WORDS = 12


def colliders(blob, tag, links=None):
    """indices of the colliders with tag name `tag` (TAGS), ascending; links: keep those on these PyBullet link indices (AGX_C_LINK, -1 = the
    base).  Both genders' human colliders are included: those of the other gender report nothing in an environment (kind 0)"""
    if tag not in TAGS:
        raise ValueError('unknown collider tag %r (one of %s)' % (tag, ', '.join(sorted(TAGS))))
    if links is not None:
        links = {int(links)} if np.isscalar(links) else {int(x) for x in links}
    o, s = blob.h['OFF_COLL'], L.C['STRIDE']
    return [c for c in range(blob.h['NCOLL']) if int(blob.i[o + c * s + L.C['TAG']]) == TAGS[tag] and (links is None or int(blob.i[o + c * s + L.C['LINK']]) in links)]


def _side(blob, side):
    if isinstance(side, str):
        return colliders(blob, side)
    if isinstance(side, tuple) and len(side) == 2 and isinstance(side[0], str):
        return colliders(blob, side[0], side[1])
    out = [int(c) for c in side]
    if any(c < 0 or c >= blob.h['NCOLL'] for c in out):
        raise ValueError('a collider index outside [0, %d)' % blob.h['NCOLL'])
    return out


def expand(blob, queries):
    """int32 [npairs, 3] rows (collider a, collider b, query id): per query the cross product of its two sides, a major, without pairs on one
    body and without a == b"""
    o, s = blob.h['OFF_COLL'], L.C['STRIDE']
    body = [int(blob.i[o + c * s + L.C['BODY']]) for c in range(blob.h['NCOLL'])]
    rows = []
    for q, (A, B) in enumerate(queries):
        sb = _side(blob, B)
        rows += [(a, b, q) for a in _side(blob, A) for b in sb if a != b and body[a] != body[b]]
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


class ProximityQuery:
    """query = ProximityQuery(env, [('tool', 'human'), (('robot', [5, 6]), 'table')], distance=0.1)
    query.closest()  -> dict(distance [n, npairs], point_a [n, npairs, 3], point_b, normal (from B towards A), kind int32 [n, npairs])
    query.nearest()  -> the same per query ([n, nqueries, ...]) plus pair int32 [n, nqueries], the winning row of .pairs (-1: nothing within reach)
    torch tensors in the GPU's memory; distance = +inf and kind = 0 where nothing is reported (beyond `distance`, a human collider of the other
    gender).  env: a vec env (its .stepper) or a Stepper; each side of a query a tag name, a (tag, links) tuple or a list of collider indices.
    A stepper holds one pair list: the query that ran last owns it, and another query's next call puts its own list back."""

    def __init__(self, env, queries, distance=4.0):
        self.stepper = getattr(env, 'stepper', env)
        self.blob = self.stepper.blob
        self.distance = float(distance)
        self.queries = list(queries)
        self.pairs = expand(self.blob, self.queries)
        if not 1 <= len(self.queries) <= 16:
            raise ValueError('1 to 16 queries')
        if len(self.pairs) == 0:
            raise ValueError('the queries name no pair of colliders on different bodies')
        self._bind()

    def _bind(self):
        if getattr(self.stepper, '_proximity_owner', None) is not self:
            self.stepper.proximity_set(self.pairs, len(self.queries))
            self.stepper._proximity_owner = self

    def _run(self, envs, per_pair):
        import torch
        st = self.stepper
        self._bind()
        ids = list(range(st.n_envs)) if envs is None else [int(e) for e in envs]
        dev = 'cuda:%d' % st.device
        n = len(ids)
        rec = torch.empty((n, len(self.pairs) if per_pair else len(self.queries), RECORD_WORDS), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        k = 0
        while k < n:                                    # one launch per run of consecutive indices
            m = k + 1
            while m < n and ids[m] == ids[m - 1] + 1:
                m += 1
            st.proximity(self.distance, records=rec[k:m] if per_pair else None, nearest=None if per_pair else rec[k:m], env0=ids[k], stream=stream)
            k = m
        out = dict(distance=rec[..., 0], point_a=rec[..., 1:4], point_b=rec[..., 4:7], normal=rec[..., 7:10], kind=rec.view(torch.int32)[..., 10])
        if not per_pair:
            out['pair'] = rec.view(torch.int32)[..., 11]
        return out

    def closest(self, envs=None):
        return self._run(envs, True)

    def nearest(self, envs=None):
        return self._run(envs, False)
