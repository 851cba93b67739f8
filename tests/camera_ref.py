"""Float64 reference of the camera (agx_camera_set / agx_render, csrc/agx_render.hip; the contract is stated in include/agx.h) for
tests/test_camera_cpu.py and tests/test_gpu_camera.py: a numpy ray caster over colliders given their body frames, the frames themselves from the
oracle's forward kinematics, and the comparison the device images are held to.

What is drawn: every collider by its vertex count -- 1 a sphere, 2 a capsule, 3 and more the polytope of model/cloth.py hull_planes(vertices) with
every plane pushed outward by the collider's radius -- for the environment's gender only (the human ranges of the blob's meta data: an independent
source, the device derives the same from the pair table), then the water particles as spheres.  A convex solid meets a ray in an interval
[t_in, t_out]; its hit is t_in, or t_out where t_in < near; the nearest hit with near <= t <= far wins, the lower index on a tie.  The ray
direction is not normalised (pixel_rays of assistive_gym_amd/camera.py), so t is the view-space depth.

Comparison (compare): the reference casts five rays per pixel -- the centre, +-JITTER pixel in x and in y.  A pixel is unsafe where the five
disagree on the hit index and is left out.  On every other pixel seg is equal, |depth - t_0| <= 0.1 max_k |t_k - t_0| + 64 2^-24 max(1, t_0),
and rgba is within 2 levels unless the five rays hit different faces of the same hull (a crease).  The jitter of 0.01 pixel is about 1.6e-4 rad at
the sizes tested, against float32 ray and frame errors of about 1e-5 rad-equivalent: a silhouette or crease the device puts on the other
side of a pixel centre lies between the jittered rays."""
import numpy as np

from assistive_gym_amd.camera import FAR, NEAR, pixel_rays, view_from_eye
from assistive_gym_amd.model import compiler as L
from assistive_gym_amd.model import xform as X
from assistive_gym_amd.model.cloth import hull_planes

U = 2.0 ** -24
JITTER = 0.01
OFFSETS = ((0.0, 0.0), (JITTER, 0.0), (-JITTER, 0.0), (0.0, JITTER), (0.0, -JITTER))
MAX_UNSAFE, MAX_CREASE, MIN_HIT = 0.05, 0.10, 0.25
BIG = 1e300

# the cameras and image sizes of the image tests: the reference's default camera; an odd size whose tiles end inside the image; for the drinking
# scene a camera near the cup, so that the water is visible (cup_camera)
CASES = {'feeding_jaco': dict(eye=(0.5, -0.75, 1.5), target=(-0.2, 0.0, 0.75), fov=60.0, width=48, height=36),
         'scratch_itch_pr2': dict(eye=(0.5, -0.75, 1.5), target=(-0.2, 0.0, 0.75), fov=60.0, width=33, height=17)}


def cup_camera(blob, state):
    """looks down into the cup of this state from 30 cm above it (5 mm particles: a narrow field of view)"""
    cup = blob.view(np.asarray(state, dtype=np.float32).reshape(1, -1))['free'][0, blob.h['TOOL_BODY'], :3].astype(np.float64)
    return dict(eye=tuple(np.round(cup + (0.0, -0.05, 0.32), 2)), target=tuple(np.round(cup + (0.0, 0.0, 0.02), 2)), fov=30.0, width=40, height=30)


class Scene:
    """colliders: list of dict(verts float64 [nv, 3], radius, tag, body) in index order; genders[c]: bit 0 drawn for a male, bit 1 for a female
    human; particle_radius: of the water particles, or None"""

    def __init__(self, colliders, genders=None, particle_radius=None):
        self.colliders = colliders
        self.ncoll = len(colliders)
        self.genders = np.full(self.ncoll, 3) if genders is None else np.asarray(genders)
        self.particle_radius = particle_radius
        self.planes = [hull_planes(c['verts']) if len(c['verts']) >= 3 else None for c in colliders]

    @classmethod
    def of_blob(cls, blob):
        cols = [blob.collider(c) for c in range(blob.h['NCOLL'])]
        g = np.full(len(cols), 3)
        rg = blob.meta['ranges']
        g[rg['human_male'][0]:rg['human_male'][1]] = 1
        g[rg['human_female'][0]:rg['human_female'][1]] = 2
        pr = None
        oc = blob.h.get('OFF_CLOTH', 0)
        if oc and int(blob.i[oc + L.CL['PARTICLES']]):
            pr = float(blob.f[oc + int(blob.i[oc + L.CL['OFF_PARAM']]) + L.CP['MARGIN']])
        return cls(cols, g, pr)


def _pick(t_in, t_out, near, far):
    """-> (t of the hit or BIG, which end: 1 entry, 2 exit, 0 none)"""
    first = (t_in >= near) & (t_in <= far)
    second = (t_in < near) & (t_out >= near) & (t_out <= far)
    return np.where(first, t_in, np.where(second, t_out, BIG)), np.where(first, 1, np.where(second, 2, 0))


def _sphere_interval(o, d, r):
    """ray o + t d against the sphere of radius r about the origin -> (t_in, t_out), an empty interval (BIG, -BIG) on a miss"""
    dd = np.sum(d * d, -1)
    t0 = -np.sum(o * d, -1) / dd
    m = o + t0[..., None] * d
    h = (r * r - np.sum(m * m, -1)) / dd
    s = np.sqrt(np.maximum(h, 0.0))
    return np.where(h >= 0, t0 - s, BIG), np.where(h >= 0, t0 + s, -BIG)


def _cylinder_interval(o, d, hv, r):
    """... against the cylinder of radius r about the segment -hv .. +hv"""
    dd, hh = np.sum(d * d, -1), float(hv @ hv)
    hd, ho = d @ hv, o @ hv
    a = hh * dd - hd * hd
    b = hh * np.sum(o * d, -1) - ho * hd
    c = hh * np.sum(o * o, -1) - ho * ho - r * r * hh
    par = a <= 1e-24 * hh * dd
    h = b * b - a * c
    s = np.sqrt(np.maximum(h, 0.0))
    with np.errstate(divide='ignore', invalid='ignore'):
        lo = np.where(par, -BIG, (-b - s) / a)
        hi = np.where(par, BIG, (-b + s) / a)
        ok = np.where(par, c <= 0, h >= 0)
        ta, tb = (-hh - ho) / hd, (hh - ho) / hd
    flat = hd == 0
    lo = np.where(flat, lo, np.maximum(lo, np.minimum(ta, tb)))
    hi = np.where(flat, hi, np.minimum(hi, np.maximum(ta, tb)))
    ok = ok & np.where(flat, np.abs(ho) <= hh, True) & (lo <= hi)
    return np.where(ok, lo, BIG), np.where(ok, hi, -BIG)


def cast(scene, frames, gender, eye, dirs, near=NEAR, far=FAR, water=None):
    """frames: float64 [ncoll, 12] position and rotation (row-major) of every collider's body; dirs: [N, 3] world ray directions; water: [npart, 3].
    -> (t [N] (far where nothing is hit), index [N] (-1 = background), outward normal [N, 3] world, face [N] (plane of a hull, -1 otherwise))"""
    n = len(dirs)
    best_t, best = np.full(n, BIG), np.full(n, -1)
    normal, face = np.zeros((n, 3)), np.full(n, -1)
    eye = np.asarray(eye, dtype=np.float64)
    old = np.seterr(all='ignore')
    for c, col in enumerate(scene.colliders):
        if not (scene.genders[c] >> (1 if gender == 1 else 0)) & 1:
            continue
        p, R = frames[c, :3], frames[c, 3:].reshape(3, 3)
        o, d = R.T @ (eye - p), dirs @ R
        v, r = col['verts'], col['radius']
        f = None
        if len(v) == 1:
            oc = o - v[0]
            t_in, t_out = _sphere_interval(oc, d, r)
            t, end = _pick(t_in, t_out, near, far)
            nb = (oc + t[:, None] * d) / r
        elif len(v) == 2:
            mid, hv = 0.5 * (v[0] + v[1]), 0.5 * (v[1] - v[0])
            oc = o - mid
            parts = [_sphere_interval(oc + hv, d, r), _sphere_interval(oc - hv, d, r)] + ([_cylinder_interval(oc, d, hv, r)] if hv @ hv > 0 else [])
            t_in, t_out = np.min([q[0] for q in parts], 0), np.max([q[1] for q in parts], 0)
            t, end = _pick(t_in, t_out, near, far)
            x = oc + t[:, None] * d
            u = np.clip((x @ hv) / (hv @ hv), -1.0, 1.0) if hv @ hv > 0 else np.zeros(n)
            nb = (x - u[:, None] * hv) / r
        else:
            pl = scene.planes[c]
            den, num = d @ pl[:, :3].T, pl[:, 3] + r - pl[:, :3] @ o
            with np.errstate(divide='ignore', invalid='ignore'):
                tt = num / den
            tin_all, tout_all = np.where(den < 0, tt, -BIG), np.where(den > 0, tt, BIG)
            f_in, f_out = np.argmax(tin_all, 1), np.argmin(tout_all, 1)
            t_in, t_out = tin_all[np.arange(n), f_in], tout_all[np.arange(n), f_out]
            outside = np.any((den == 0) & (num < 0), 1) | (t_in > t_out)
            t, end = _pick(np.where(outside, BIG, t_in), np.where(outside, -BIG, t_out), near, far)
            f = np.where(end == 2, f_out, f_in)
            nb = pl[f, :3]
        win = (end > 0) & (t < best_t)
        best_t[win], best[win] = t[win], c
        normal[win] = (nb @ R.T)[win]
        face[win] = f[win] if f is not None else -1
    if water is not None and scene.particle_radius:
        for k, w in enumerate(np.asarray(water, dtype=np.float64)):
            oc = eye - w
            t_in, t_out = _sphere_interval(oc, dirs, scene.particle_radius)
            t, end = _pick(t_in, t_out, near, far)
            win = (end > 0) & (t < best_t)
            best_t[win], best[win] = t[win], scene.ncoll + k
            normal[win] = ((oc + t[:, None] * dirs) / scene.particle_radius)[win]
            face[win] = -1
    np.seterr(**old)
    return np.where(best >= 0, best_t, far), best, normal, face


def shade(scene, index, normal, colours, light, ambient, diffuse):
    """rgba uint8 [N, 4] of hits (index, normal): round(255 min(1, colour (ambient + diffuse max(0, n . l)))), the background unshaded"""
    l = np.asarray(light, dtype=np.float64)
    l = l / np.linalg.norm(l)
    tags = np.array([c['tag'] if 1 <= c['tag'] <= 9 else 0 for c in scene.colliders] + [10], dtype=int)
    ci = np.where(index < 0, 11, tags[np.minimum(np.maximum(index, 0), scene.ncoll)])
    s = np.where(index < 0, 1.0, ambient + diffuse * np.maximum(0.0, normal @ l))
    rgb = np.round(255.0 * np.minimum(1.0, np.asarray(colours, dtype=np.float64)[ci] * s[:, None]))
    return np.concatenate([rgb, np.full((len(index), 1), 255.0)], 1).astype(np.uint8)


class Camera:
    """the view of agx_camera_set as the device receives it: eye, target and up rounded to float32 first"""

    def __init__(self, eye, target, up=(0.0, 0.0, 1.0), fov=60.0, width=48, height=36, near=NEAR, far=FAR):
        self.eye, self.target, self.up = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (eye, target, up))
        self.fov, self.width, self.height = float(np.float32(fov)), width, height
        self.near, self.far = float(np.float32(near)), float(np.float32(far))
        self.basis = view_from_eye(self.eye, self.target, self.up)

    def rays(self, di=0.0, dj=0.0):
        return pixel_rays(self.basis, self.fov, self.width, self.height, di, dj).reshape(-1, 3)


def render_five(scene, cam, frames, gender, water=None):
    """the five casts of one environment's image -> list of (t, index, normal, face), the centre ray first"""
    return [cast(scene, frames, gender, cam.eye, cam.rays(di, dj), cam.near, cam.far, water) for di, dj in OFFSETS]


def masks(five):
    """-> (safe [N]: the five rays agree on the hit index; crease [N]: safe, but they hit different faces of a hull; hit [N])"""
    idx = np.stack([f[1] for f in five]); fc = np.stack([f[3] for f in five])
    safe = np.all(idx == idx[0], 0)
    crease = safe & np.any(fc != fc[0], 0)
    return safe, crease, idx[0] >= 0


def check_caps(five, label=''):
    safe, crease, hit = masks(five)
    n = len(safe)
    shares = dict(unsafe=1.0 - safe.sum() / n, crease=crease.sum() / n, hit=hit.sum() / n)
    print('%s: unsafe %.2f %%, crease %.2f %%, hit %.1f %%' % (label, 100 * shares['unsafe'], 100 * shares['crease'], 100 * shares['hit']))
    assert shares['unsafe'] <= MAX_UNSAFE and shares['crease'] <= MAX_CREASE and shares['hit'] >= MIN_HIT, (label, shares)
    return shares


def compare(scene, cam, five, colours, light, ambient, diffuse, depth, seg, rgba, worst, label=''):
    """device images of one environment (flattened or [h, w]) against the five casts; updates worst = dict(depth=, rgba=) with the largest
    error / bound ratios"""
    check_caps(five, label)
    safe, crease, hit = masks(five)
    t0, i0, n0, _ = five[0]
    seg, depth, rgba = np.asarray(seg).reshape(-1), np.asarray(depth, dtype=np.float64).reshape(-1), np.asarray(rgba).reshape(-1, 4)
    assert np.array_equal(seg[safe], i0[safe]), (label, 'seg differs on %d safe pixels' % int((seg[safe] != i0[safe]).sum()))
    spread = np.max(np.abs(np.stack([f[0] for f in five[1:]]) - t0), 0)
    bound = 0.1 * spread + 64 * U * np.maximum(1.0, t0)
    ratio = np.abs(depth - t0)[safe] / bound[safe]
    want = shade(scene, i0, n0, colours, light, ambient, diffuse)
    keep = safe & ~crease
    dl = np.abs(rgba.astype(int) - want.astype(int))[keep]
    worst['depth'] = max(worst.get('depth', 0.0), float(ratio.max()))
    worst['rgba'] = max(worst.get('rgba', 0.0), float(dl.max()) / 2.0)
    print('%s: worst |depth error| / bound %.3g, worst rgba difference %d levels (of 2)' % (label, ratio.max(), dl.max()))
    assert ratio.max() <= 1.0, (label, 'depth', float(ratio.max()))
    assert dl.max() <= 2, (label, 'rgba', int(dl.max()))


# ---- collider frames from the oracle's forward kinematics --------------------------------------------------------------------------------------
def ref_frames(blob, oracle, state):
    """float64 [ncoll, 12] of one float32 state record, and per collider the number of chain levels behind its rotation and the reach behind its
    position (frame_bounds): links from oracle.fk, the base / free bodies / static human bodies from their records"""
    v = blob.view(np.asarray(state, dtype=np.float32).reshape(1, -1).copy())
    pos, rot = oracle.fk(np.asarray(state, dtype=np.float32).copy())
    gender = int(v['gender'][0])
    base_reach = float(np.linalg.norm(v['base'][0, :3]))
    hbase_reach = float(np.linalg.norm(v['human'][0, 0, :3])) if blob.nhuman else 0.0
    levels, reach = np.zeros(blob.ndof, dtype=int), np.zeros(blob.ndof)
    for d in range(blob.ndof):
        par = blob.robot_i(d, 'PARENT', gender)
        step = float(np.linalg.norm(blob.robot_f(d, 'TPOS', 3, gender))) + (abs(float(v['q'][0, d])) if blob.robot_i(d, 'JTYPE', gender) == 1 else 0.0)
        levels[d] = 1 + (levels[par] if par >= 0 else 1)
        reach[d] = step + (reach[par] if par >= 0 else (hbase_reach if par == -2 else base_reach))
    out = np.zeros((blob.h['NCOLL'], 12)); lev = np.zeros(blob.h['NCOLL'], dtype=int); rch = np.zeros(blob.h['NCOLL'])
    for c in range(blob.h['NCOLL']):
        code = blob.collider(c)['body']
        if code == -1:
            p, R, k, r = np.zeros(3), np.eye(3), 0, 0.0
        elif code >= 300:
            rec = v['human'][0, code - 300].astype(np.float64); p, R, k, r = rec[:3], X.quat_to_mat(rec[3:7] / np.linalg.norm(rec[3:7])), 1, 0.0
        elif code >= 200:
            rec = v['free'][0, code - 200].astype(np.float64); p, R, k, r = rec[:3], X.quat_to_mat(rec[3:7] / np.linalg.norm(rec[3:7])), 1, 0.0
        elif code == 100:
            rec = v['base'][0].astype(np.float64); p, R, k, r = rec[:3], X.quat_to_mat(rec[3:7] / np.linalg.norm(rec[3:7])), 1, 0.0
        else:
            p, R, k, r = pos[code], rot[code], levels[code], reach[code]
        out[c, :3], out[c, 3:] = p, np.asarray(R).reshape(9)
        lev[c], rch[c] = k, r
    return out, lev, rch


ROT_LEVEL = 48      # roundings per chain level on an entry of the rotation, see frame_bounds


def frame_bounds(levels, reach):
    """float32 rounding bounds of the device's frames (csrc/agx_dyn.h kinematics, csrc/agx_ctx.h body_xf) against ref_frames, per collider:
    (bound on every position component, bound on every rotation entry).
    A chain level is R = (PR Rt) A(q), p = PR tp + pp.  Rt comes from a float32 quaternion: a square root and a division on every component (4 u),
    entries 1 - 2 (y^2 + z^2) of at most 6 roundings -- 10 u; the axis-angle matrix: sine and cosine at 2 ulp and Rodrigues' terms, 8 u; a 3 x 3
    product of matrices with unit rows and columns adds 3 u per entry (sum_k |a_ik| |b_kj| <= 1).  That is 24 u per level and entry, taken twice
    because an entry's error is held to the bound on the matrix norm that carries over to the next level: ROT_LEVEL = 48 u per level.  A body
    whose rotation is one quaternion (base, free and human bodies) is one level, and its position is a copy: bound 0.
    The position of level k: the rotation error of the parent, at most sqrt(3) ROT_LEVEL (k - 1) u in norm, acts on the offset tp, the product
    and the sum add 4 u |p|; summed over the chain both are below (sqrt(3) ROT_LEVEL + 4) k u reach, reach = |base position| + the chain's offsets."""
    levels, reach = np.asarray(levels, dtype=np.float64), np.asarray(reach, dtype=np.float64)
    return (np.sqrt(3.0) * ROT_LEVEL + 4.0) * levels * U * reach, ROT_LEVEL * levels * U
