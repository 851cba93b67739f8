"""The batched camera: depth, segmentation and RGB images of the environments of a vec env (or a bare Stepper), ray-cast on the device
(csrc/agx_render.hip through agx_camera_set / agx_render, include/agx.h).

The reference's env.setup_camera / setup_camera_rpy / get_camera_image_depth (assistive_gym/envs/env.py:342-359) hand a view to PyBullet's renderer.
Here one camera is shared by all environments -- every scene sits at the same world coordinates -- and what is drawn is the COLLISION geometry of the
model blob: spheres, capsules and convex hulls (their face planes pushed outward by the collider's radius), coloured by the collider's tag, plus the
water particles of a drinking scene and, where it is switched on (garment=True / set_garment; off by default), the garment of a dressing scene:
its triangles at their current node positions, both sides visible, flat shaded in the gown's own colour (139, 195, 74) / 256, opaque; face f has
the segmentation value collider count + f (Stepper.garment_faces).  Not drawn: visual meshes and textures, shadows, a specular term, the gown's
translucency.  The images are not PyBullet's pixel for pixel.

The view conventions live here, once: view_from_eye / view_from_rpy (PyBullet's computeViewMatrix / computeViewMatrixFromYawPitchRoll with the
z axis up), pixel_rays (the ray of a pixel) and bullet_depth (the depth buffer PyBullet returns for a metric depth)."""
import numpy as np

NEAR, FAR = 0.01, 100.0                      # env.py:346
DEFAULT_EYE, DEFAULT_TARGET, DEFAULT_FOV = (0.5, -0.75, 1.5), (-0.2, 0.0, 0.75), 60.0      # env.py:342
DEFAULT_LIGHT, DEFAULT_AMBIENT, DEFAULT_DIFFUSE = (0.0, -3.0, 1.0), 0.8, 0.3                # env.py:354


def view_from_eye(eye, target, up=(0.0, 0.0, 1.0)):
    """p.computeViewMatrix: rows right, up, forward of the camera in world coordinates, float64 [3, 3] (forward = the view direction, -z of the camera)"""
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    f = target - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, up)
    s = s / np.linalg.norm(s)
    return np.stack([s, np.cross(s, f), f])


def view_from_rpy(target, distance, yaw, pitch, roll):
    """p.computeViewMatrixFromYawPitchRoll(target, distance, yaw, pitch, roll, upAxisIndex=2), angles in degrees -> (eye, target, up): the camera
    sits at target + R (0, -distance, 0) with up vector R (0, 0, 1), R = Rz(yaw) Ry(roll) Rx(pitch)"""
    y, p, r = np.radians([yaw, pitch, roll])
    Rz = np.array([[np.cos(y), -np.sin(y), 0.0], [np.sin(y), np.cos(y), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(r), 0.0, np.sin(r)], [0.0, 1.0, 0.0], [-np.sin(r), 0.0, np.cos(r)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(p), -np.sin(p)], [0.0, np.sin(p), np.cos(p)]])
    R = Rz @ Ry @ Rx
    target = np.asarray(target, dtype=np.float64)
    return target + R @ np.array([0.0, -float(distance), 0.0]), target, R @ np.array([0.0, 0.0, 1.0])


def pixel_rays(basis, fov, width, height, di=0.0, dj=0.0):
    """world directions of the rays through the pixel centres (shifted by di, dj pixels), float64 [height, width, 3]: in camera space
    ((2 (i + 0.5) / w - 1) aspect tan(fov / 2), (1 - 2 (j + 0.5) / h) tan(fov / 2), -1), row 0 at the top; not normalised, so the ray parameter is
    the view-space depth"""
    ty = np.tan(0.5 * np.radians(float(fov)))
    tx = ty * width / height
    x = (2.0 * (np.arange(width) + 0.5 + di) / width - 1.0) * tx
    y = (1.0 - 2.0 * (np.arange(height) + 0.5 + dj) / height) * ty
    return x[None, :, None] * basis[0] + y[:, None, None] * basis[1] + basis[2]


def bullet_depth(z, near=NEAR, far=FAR):
    """the depth buffer PyBullet's getCameraImage returns for the view-space depth z: far (z - near) / (z (far - near)), 0 at the near plane, 1 at the far plane"""
    return far * (z - near) / (z * (far - near))


def collider_info(blob, index):
    """what a value of the segmentation image stands for: (tag, body code, link) of collider `index` -- AGX_C_TAG, AGX_C_BODY, AGX_C_LINK of
    include/agx_blob.h -- ('water', k, -1) for particle k of a drinking scene (index = collider count + k), ('garment', f, -1) for face f of the
    garment of a dressing scene (index = collider count + f), None for the background (-1)"""
    ncoll = blob.h['NCOLL']
    if index < 0:
        return None
    if index >= ncoll:
        from .model import compiler as L
        oc = blob.h.get('OFF_CLOTH', 0)
        garment = bool(oc) and not int(blob.i[oc + L.CL['PARTICLES']])
        return ('garment' if garment else 'water', int(index) - ncoll, -1)
    c = blob.collider(int(index))
    return (c['tag'], c['body'], c['link'])


class BatchedCamera:
    """camera = BatchedCamera(env, 64, 48); images = camera.render()        # every environment
    images = camera.render(range(16))                                       # a subset (a contiguous range is one launch)
    -> dict(depth float32 [n, h, w] metric view-space depth, `far` where nothing is hit; seg int32 [n, h, w] collider index (collider_info), -1 =
    background; rgba uint8 [n, h, w, 4]), torch tensors in the GPU's memory.  env: a vec env (its .stepper) or a Stepper.
    garment=True draws the garment of a dressing scene (seg = collider count + face); a scene without one raises."""

    def __init__(self, env, width=1920 // 4, height=1080 // 4, camera_eye=DEFAULT_EYE, camera_target=DEFAULT_TARGET, fov=DEFAULT_FOV,
                 light_pos=DEFAULT_LIGHT, ambient=DEFAULT_AMBIENT, diffuse=DEFAULT_DIFFUSE, garment=False):
        self.stepper = getattr(env, 'stepper', env)
        self.blob = self.stepper.blob
        self.width, self.height = int(width), int(height)
        self.light_pos, self.ambient, self.diffuse = tuple(light_pos), float(ambient), float(diffuse)
        self.setup(camera_eye, camera_target, fov)
        self.garment = False
        if garment:
            self.set_garment(True)

    def set_garment(self, on=True):
        """draw the garment of a dressing scene, or stop drawing it (agx_camera_garment)"""
        self.stepper.camera_garment(on)
        self.garment = bool(on)

    def setup(self, camera_eye=DEFAULT_EYE, camera_target=DEFAULT_TARGET, fov=DEFAULT_FOV, up=(0.0, 0.0, 1.0)):
        """env.setup_camera (env.py:342-346)"""
        self.eye, self.target, self.up, self.fov = tuple(camera_eye), tuple(camera_target), tuple(up), float(fov)
        self.stepper.camera_set(self.eye, self.target, self.up, self.fov, self.width, self.height, NEAR, FAR)

    def setup_rpy(self, camera_target=DEFAULT_TARGET, distance=1.5, rpy=(0, -35, 40), fov=DEFAULT_FOV):
        """env.setup_camera_rpy (env.py:348-352): rpy = (roll, pitch, yaw) in degrees"""
        eye, target, up = view_from_rpy(camera_target, distance, rpy[2], rpy[1], rpy[0])
        self.setup(eye, target, fov, up)

    def render(self, envs=None, light_pos=None, ambient=None, diffuse=None):
        import torch
        st = self.stepper
        ids = list(range(st.n_envs)) if envs is None else [int(e) for e in envs]
        dev = 'cuda:%d' % st.device
        n, h, w = len(ids), self.height, self.width
        out = dict(depth=torch.empty((n, h, w), dtype=torch.float32, device=dev), seg=torch.empty((n, h, w), dtype=torch.int32, device=dev),
                   rgba=torch.empty((n, h, w, 4), dtype=torch.uint8, device=dev))
        stream = torch.cuda.current_stream(dev).cuda_stream
        k = 0
        while k < n:                                    # one launch per run of consecutive indices
            m = k + 1
            while m < n and ids[m] == ids[m - 1] + 1 and m - k < 65535:
                m += 1
            st.render(ids[k], m - k, light_pos if light_pos is not None else self.light_pos, self.ambient if ambient is None else ambient,
                      self.diffuse if diffuse is None else diffuse, out['depth'][k:m], out['seg'][k:m], out['rgba'][k:m], stream=stream)
            k = m
        return out
