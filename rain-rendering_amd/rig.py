"""Camera rigs for the RIG particle model (tools/particles.py, rr_set_particle_rig): several cameras that look at one rain field.

    rig = Rig.stereo(0.54)                                   # KITTI's documented baseline; view 0 left, view 1 right
    rig = Rig.yaw_ring([0, 55, 110, 180, -110, -55], 0.8)    # a surround ring from the user's own calibration
    rig = Rig([(R0, c0), (R1, c1)])                          # rotations rig -> camera and camera centres in the rig frame

The rig frame is the single camera's frame of the other models: x right, y up, looking along -z; the vehicle's motion gives the
drops +speed in z.  A view is p_cam = R (p_rig - c).  All views share the dataset's intrinsics.  Put the rig's origin at the
mean height of the cameras (and between them): the slots' boxes are centred on the origin and grow by max |c.y| in height
(`box`), and every slot in a box that no view sees is evaluated for nothing.  The presets do so.

Every transcendental (yaw, pitch -> R) is evaluated here, on the host; the library and the numpy statement get matrices."""
import json

import numpy as np

MAX_VIEWS = 8
ORTHO_TOL = 1e-12            # |R R^T - I| and |det R - 1|: sixteen roundings of products of numbers <= 1 stay far below it


def _rot_y(deg):
    a = np.deg2rad(float(deg))
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rot_x(deg):
    a = np.deg2rad(float(deg))
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def check_views(views):
    """The refusals of rr_set_particle_rig for the views, as ValueError: 1..8 views, finite numbers, R orthonormal with
    determinant +1 within ORTHO_TOL.  Returns [(R [3, 3], c [3])]."""
    try:
        views = [(np.array(R, np.float64).reshape(3, 3), np.array(c, np.float64).reshape(3)) for R, c in views]
    except (TypeError, ValueError):
        raise ValueError("a rig is a list of (R [3 x 3], c [3]) views")
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError("a rig has 1 to %d views, got %d" % (MAX_VIEWS, len(views)))
    for v, (R, c) in enumerate(views):
        if not (np.all(np.isfinite(R)) and np.all(np.isfinite(c))):
            raise ValueError("view %d: R and c must be finite" % v)
        if np.abs(R @ R.T - np.eye(3)).max() > ORTHO_TOL or abs(np.linalg.det(R) - 1.0) > ORTHO_TOL:
            raise ValueError("view %d: R is not orthonormal with determinant +1 (within %g)" % (v, ORTHO_TOL))
    return views


def check_active(active, n_views):
    """The active list of rr_set_particle_rig: 1..n_views distinct view numbers."""
    if active is None:
        return list(range(n_views))
    raw = np.atleast_1d(np.asarray(active)).reshape(-1).tolist()
    ok = bool(raw) and all(not isinstance(v, bool) and isinstance(v, (int, float)) and v == int(v) for v in raw)
    a = [int(v) for v in raw] if ok else []
    if not ok or len(set(a)) != len(a) or any(v < 0 or v >= n_views for v in a):
        raise ValueError("views must be distinct numbers in 0..%d, got %r" % (n_views - 1, active))
    return a


class Rig:
    def __init__(self, views):
        self.views = check_views(views)

    def __len__(self):
        return len(self.views)

    @classmethod
    def stereo(cls, baseline_m):
        """Two parallel cameras `baseline_m` apart along x, the origin midway: view 0 is the left camera, view 1 the right."""
        b = float(baseline_m)
        if not (np.isfinite(b) and b > 0):
            raise ValueError("stereo baseline must be positive and finite (metres), got %r" % (baseline_m,))
        eye = np.eye(3)
        return cls([(eye, [-0.5 * b, 0.0, 0.0]), (eye, [0.5 * b, 0.0, 0.0])])

    @classmethod
    def yaw_ring(cls, yaws_deg, radius_m, height_m=0, pitches_deg=None):
        """Cameras on a horizontal circle of `radius_m` around the origin at `height_m`, each looking outward along its yaw
        (degrees, counter-clockwise seen from above: 0 looks along -z like the single camera, +90 along -x, to the left);
        `pitches_deg`: per camera, positive looks up.  height_m is the cameras' height above the rig's origin: leave it 0."""
        yaws = [float(y) for y in np.atleast_1d(yaws_deg)]
        pitches = [0.0] * len(yaws) if pitches_deg is None else [float(p) for p in np.atleast_1d(pitches_deg)]
        if len(pitches) != len(yaws):
            raise ValueError("%d pitches for %d yaws" % (len(pitches), len(yaws)))
        views = []
        for yaw, pitch in zip(yaws, pitches):
            to_rig = _rot_y(yaw) @ _rot_x(pitch)               # camera -> rig
            fwd = _rot_y(yaw) @ np.array([0.0, 0.0, -1.0])
            views.append((to_rig.T, float(radius_m) * fwd + np.array([0.0, float(height_m), 0.0])))
        return cls(views)

    @classmethod
    def from_spec(cls, spec):
        """The driver's --rig: 'mono' (one identity view: a single camera, so that it can have a trajectory),
        'stereo:<baseline in metres>' or the path of a JSON file {"views": [{"R": [9 or 3 x 3], "c": [3]}, ...]}."""
        if isinstance(spec, Rig):
            return spec
        spec = str(spec)
        if spec == 'mono':
            return cls([(np.eye(3), [0.0, 0.0, 0.0])])
        if spec.startswith('stereo:'):
            try:
                return cls.stereo(float(spec[len('stereo:'):]))
            except ValueError as e:
                raise ValueError("--rig %s: %s" % (spec, e))
        with open(spec) as fh:
            doc = json.load(fh)
        if any(k not in ('R', 'c') for v in doc['views'] for k in v):
            raise ValueError("%s: a view holds R and c only (per-view intrinsics are not supported)" % spec)
        return cls([(v['R'], v['c']) for v in doc['views']])

    def box(self, cam, margin=0.05):
        """(r, r_y, o_y) of the slots' boxes for a camera with cam.W, cam.H, cam.fpx: over the four far corners
        (+-hx, +-hy, -1) of every view's margin-enlarged frustum at unit depth, turned into the rig frame, r = the largest |x|
        or |z| and r_y = the largest |y|; o_y = max |c.y|.  A frustum is the convex hull of its apex and far corners, so view v's
        frustum up to z_max lies within +-r z_max of c_v in x and z (inside the lattice cell centred on the camera: the view
        cannot see a slot twice, and the nearest image is the only one it can see) and within +-(r_y z_max + o_y) in y."""
        hx, hy = ((0.5 + margin) * float(cam.W)) / cam.fpx, ((0.5 + margin) * float(cam.H)) / cam.fpx
        r = r_y = o_y = 0.0
        for R, c in self.views:
            for sx in (-1.0, 1.0):
                for sy in (-1.0, 1.0):
                    d = R.T @ np.array([sx * hx, sy * hy, -1.0])
                    r = max(r, abs(float(d[0])), abs(float(d[2])))
                    r_y = max(r_y, abs(float(d[1])))
            o_y = max(o_y, abs(float(c[1])))
        return r, r_y, o_y

    def as_records(self):
        """The views as RIG_VIEW_DTYPE records (rr_rig_view)."""
        from . import hip_backend
        out = np.zeros(len(self.views), hip_backend.RIG_VIEW_DTYPE)
        for v, (R, c) in enumerate(self.views):
            out[v]['R'] = R.reshape(9)
            out[v]['c'] = c
        return out
