"""Camera trajectories for the RIG particle model (tools/particles.py, rr_set_particle_trajectory): one rain field seen from a
rig that moves and turns.

    traj = Trajectory.from_file('poses/07.txt', hz=10)            # KITTI odometry poses.txt: 12 numbers per line
    traj = Trajectory(poses [N, 3, 4] or [N, 4, 4], hz, 'native') # camera (rig) -> world, the project's own frame
    poses = traj.compose(Rig.stereo(0.54), exposure_s)            # [N, V] POSE_DTYPE records: what the library receives
    box = traj.box(rig, cam, margin)                              # the slots' box of the run

A pose is the rig's frame in the world: p_world = R p_rig + t.  Conventions: 'native' is the project's own frame (x right, y
up, looking along -z: the rig frame of rig.py); 'kitti' is the KITTI odometry layout (x right, y down, z forward), converted
by S Q S with S = diag(1, -1, -1).  Row f of a trajectory is time index f (rendered frame f) at t = f / hz.

`compose` gives every (instant, view) two world -> camera poses, p_cam = R (p_world - c): (R0, c0) at t_k and (R1, c1) at
t_k + exposure.  The end pose is the fraction exposure * hz of the way to pose k + 1: the translation linearly, the rotation
as R_k exp(f log(R_k^T R_k+1)) (Rodrigues); the last pose extrapolates from k - 1; a single pose stands still.  Where two
consecutive poses are equal bit for bit the end pose IS the start pose, bit for bit: the rig model's own records.

Every transcendental is evaluated here, on the host: the library and the numpy statement get matrices."""
import numpy as np

from .rig import MAX_VIEWS, ORTHO_TOL, Rig

# numpy mirror of rr_traj_pose (192 bytes)
POSE_DTYPE = np.dtype([('R0', '<f8', (9,)), ('c0', '<f8', (3,)), ('R1', '<f8', (9,)), ('c1', '<f8', (3,))], align=True)
CONVENTIONS = ('kitti', 'native')
MAX_CENTRE = 1e6               # metres: beyond it the centre's rounding (2^-53 |c|) reaches a tenth of a nanometre x 1e3
MAX_INSTANTS = 1 << 20
POSE_TOL = 1e-9                # a composed pose: the library's own tolerance (rr_set_particle_rig's)
MAX_TURN_DEG = 170.0           # between consecutive poses: the axis of a half turn is not defined
_S = np.diag([1.0, -1.0, -1.0])


def _log_so3(rel):
    """(unit axis, angle) of a rotation matrix; angle 0 gives (None, 0.0)."""
    w = 0.5 * np.array([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]])
    s = float(np.sqrt(w @ w))
    theta = float(np.arctan2(s, 0.5 * (np.trace(rel) - 1.0)))
    if s == 0.0 and theta == 0.0:
        return None, 0.0
    if theta > np.deg2rad(MAX_TURN_DEG):
        raise ValueError("consecutive poses are more than %g degrees apart" % MAX_TURN_DEG)
    return w / s, theta


def _exp_so3(axis, angle):
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _nearest_rotation(M):
    u, _, vt = np.linalg.svd(M)
    return u @ np.diag([1.0, 1.0, float(np.sign(np.linalg.det(u @ vt)))]) @ vt


class _Bound:
    """A trajectory bound to a rig, where tools/particles.py expects a rig: the rig's views, the TRAJECTORY's box."""

    def __init__(self, traj, rig):
        self.trajectory, self.rig, self.views = traj, rig, rig.views

    def __len__(self):
        return len(self.views)

    def box(self, cam, margin=0.05):
        return self.trajectory.box(self.rig, cam, margin)


class Trajectory:
    def __init__(self, poses_cam_to_world, hz, convention='native', orthonormalise=False):
        """poses_cam_to_world: [N, 3, 4] or [N, 4, 4], p_world = R p_rig + t, N >= 1; hz: poses per second (the run's cam_hz);
        convention: 'kitti' or 'native'.  ValueError, mirroring rig.check_views: a wrong shape, numbers that are not finite, an R
        that is not orthonormal with determinant +1 within rig.ORTHO_TOL, a bottom row other than (0, 0, 0, 1), |t| beyond
        1e6 m, more than 2^20 poses, hz not positive, an unknown convention.  orthonormalise: replace every R by the nearest
        rotation first (for poses read from text with a few digits; an R further than 1e-3 from a rotation is still refused)."""
        if convention not in CONVENTIONS:
            raise ValueError("trajectory convention %r: expected one of %s" % (convention, ', '.join(CONVENTIONS)))
        try:
            hz = float(hz)
        except (TypeError, ValueError):
            raise ValueError("trajectory hz must be a number, got %r" % (hz,))
        if not (np.isfinite(hz) and hz > 0):
            raise ValueError("trajectory hz must be positive and finite, got %r" % (hz,))
        try:
            P = np.array(poses_cam_to_world, np.float64)
        except (TypeError, ValueError):
            raise ValueError("a trajectory is an array of [N, 3, 4] or [N, 4, 4] poses")
        if P.ndim != 3 or P.shape[0] < 1 or P.shape[1:] not in ((3, 4), (4, 4)):
            raise ValueError("a trajectory is an array of [N, 3, 4] or [N, 4, 4] poses with N >= 1, got shape %s" % (P.shape,))
        if len(P) > MAX_INSTANTS:
            raise ValueError("a trajectory has at most 2^20 poses, got %d" % len(P))
        if not np.all(np.isfinite(P)):
            raise ValueError("pose %d: R and t must be finite" % int(np.argwhere(~np.isfinite(P))[0][0]))
        if P.shape[1] == 4 and np.any(P[:, 3] != np.array([0.0, 0.0, 0.0, 1.0])):
            raise ValueError("pose %d: the bottom row must be (0, 0, 0, 1)" % int(np.argwhere(P[:, 3] != np.array([0.0, 0.0, 0.0, 1.0]))[0][0]))
        R, t = P[:, :3, :3].copy(), P[:, :3, 3].copy()
        if orthonormalise:
            for k in range(len(R)):
                Rn = _nearest_rotation(R[k])
                if np.abs(Rn - R[k]).max() > 1e-3:
                    raise ValueError("pose %d: R is further than 1e-3 from a rotation" % k)
                R[k] = Rn
        if convention == 'kitti':
            R, t = _S @ R @ _S, t @ _S
        for k in range(len(R)):
            if np.abs(R[k] @ R[k].T - np.eye(3)).max() > ORTHO_TOL or abs(np.linalg.det(R[k]) - 1.0) > ORTHO_TOL:
                raise ValueError("pose %d: R is not orthonormal with determinant +1 (within %g)" % (k, ORTHO_TOL))
            if float(np.sqrt(t[k] @ t[k])) > MAX_CENTRE:
                raise ValueError("pose %d: |t| is beyond %g m" % (k, MAX_CENTRE))
        self.R, self.t, self.hz, self.convention = R, t, hz, convention
        self._level = False
        self._memo = {}

    def __len__(self):
        return len(self.R)

    @classmethod
    def from_file(cls, path, hz=10.0, convention='kitti', orthonormalise=True):
        """The KITTI odometry poses.txt layout: one pose per line, the 12 numbers of its 3 x 4 matrix row by row (blank lines and
        lines that start with '#' are skipped).  hz: KITTI's 10 by default.  The files carry a few digits, so every R is
        replaced by the nearest rotation unless orthonormalise=False."""
        rows = []
        with open(path) as fh:
            for ln, line in enumerate(fh, 1):
                line = line.strip()
                if not line or line.startswith('#'):
                    continue
                try:
                    v = [float(x) for x in line.split()]
                except ValueError:
                    raise ValueError("%s:%d: not a number" % (path, ln))
                if len(v) != 12:
                    raise ValueError("%s:%d: a pose has 12 numbers, got %d" % (path, ln, len(v)))
                rows.append(v)
        if not rows:
            raise ValueError("%s: no pose" % path)
        return cls(np.array(rows).reshape(-1, 3, 4), hz, convention, orthonormalise)

    def levelled(self):
        """A copy in which every pose's START altitude is removed from both of its ends: the rig stays at y = 0 at every t_k and
        keeps only its climb during the exposure.  For hilly drives, where the altitude range would enter the box (o_y) and
        multiply the slot count.  What is given up: the vertical motion of the camera BETWEEN frames -- a drop's height in
        frame k + 1 is off by the rig's climb since frame k, so the field is no longer coherent in y across such frames."""
        out = Trajectory.__new__(Trajectory)
        out.R, out.t, out.hz, out.convention = self.R, self.t, self.hz, self.convention
        out._level = True
        out._memo = {}
        return out

    def at_rate(self, hz):
        """A copy of the same poses at another rate (the driver: a row per rendered frame, at the run's cam_hz)."""
        hz = float(hz)
        if not (np.isfinite(hz) and hz > 0):
            raise ValueError("trajectory hz must be positive and finite, got %r" % (hz,))
        out = Trajectory.__new__(Trajectory)
        out.R, out.t, out.hz, out.convention, out._level, out._memo = self.R, self.t, hz, self.convention, self._level, {}
        return out

    def bind(self, rig):
        """This trajectory where tools/particles.py takes a rig (sim_frames, rig_slot_counts, rig_tables): the rig's views with
        the trajectory's box."""
        return _Bound(self, rig)

    def _ends(self, exposure_s):
        """(R_end [N, 3, 3], t_end [N, 3]) of the rig at t_k + exposure."""
        e = float(exposure_s)
        if not (np.isfinite(e) and e >= 0):
            raise ValueError("exposure must be finite and >= 0 seconds, got %r" % (exposure_s,))
        f = e * self.hz
        N = len(self.R)
        Re, te = self.R.copy(), self.t.copy()
        for k in range(N):
            if N == 1:
                break
            a, b = (k, k + 1) if k + 1 < N else (k - 1, k)
            te[k] = self.t[k] + f * (self.t[b] - self.t[a]) if np.any(self.t[b] != self.t[a]) else self.t[k]
            if np.array_equal(self.R[a], self.R[b]):
                continue
            axis, theta = _log_so3(self.R[a].T @ self.R[b])
            if axis is not None:
                Re[k] = self.R[k] @ _exp_so3(axis, f * theta)
        return Re, te

    def compose(self, rig, exposure_s):
        """[N, V] POSE_DTYPE records (R0, c0, R1, c1): world -> camera of view v at t_k and at t_k + exposure, R = R_view R_rig^T
        and c = t_rig + R_rig c_view.  ValueError if a composed pose fails the library's own checks."""
        rig = Rig.from_spec(rig)
        key = (b''.join(R.tobytes() + c.tobytes() for R, c in rig.views), float(exposure_s))
        if key in self._memo:                                   # (a run asks once per frame: the table is made once)
            return self._memo[key]
        Re, te = self._ends(exposure_s)
        out = np.zeros((len(self.R), len(rig.views)), POSE_DTYPE)
        for k in range(len(self.R)):
            lift = np.array([0.0, self.t[k][1], 0.0]) if self._level else 0.0
            for v, (Rv, cv) in enumerate(rig.views):
                o = out[k, v]
                o['R0'] = (Rv @ self.R[k].T).reshape(9)
                o['c0'] = (self.t[k] - lift) + self.R[k] @ cv
                o['R1'] = (Rv @ Re[k].T).reshape(9)
                o['c1'] = (te[k] - lift) + Re[k] @ cv
        check_poses(out)
        out.setflags(write=False)
        self._memo = {key: out}
        return out

    def box(self, rig, cam, margin=0.05):
        """(r, r_y, o_y) of the slots' boxes: Rig.box taken over every composed rotation at BOTH ends of the exposure
        (cam.exposure), and o_y = max |c.y| over all of them.  A rig that turns through every heading reaches r = sqrt(hx^2 + 1)
        and its altitude range enters o_y (see levelled)."""
        rig = Rig.from_spec(rig)
        po = self.compose(rig, cam.exposure)
        hx, hy = ((0.5 + margin) * float(cam.W)) / cam.fpx, ((0.5 + margin) * float(cam.H)) / cam.fpx
        corners = np.array([[sx * hx, sy * hy, -1.0] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)])
        Rs = np.concatenate([po['R0'].reshape(-1, 3, 3), po['R1'].reshape(-1, 3, 3)])
        d = np.abs(np.einsum('nji,cj->nci', Rs, corners))            # R^T corner
        r = float(max(d[..., 0].max(), d[..., 2].max()))
        r_y = float(d[..., 1].max())
        o_y = float(max(np.abs(po['c0'][..., 1]).max(), np.abs(po['c1'][..., 1]).max()))
        return r, r_y, o_y


def check_poses(poses):
    """The refusals of rr_set_particle_trajectory for a table of POSE_DTYPE records, as ValueError."""
    po = np.asarray(poses)
    if po.dtype != POSE_DTYPE:
        raise ValueError("a pose table holds POSE_DTYPE records")
    if po.ndim == 2 and not 1 <= po.shape[1] <= MAX_VIEWS:
        raise ValueError("a pose table has 1 to %d views per instant, got %d" % (MAX_VIEWS, po.shape[1]))
    if len(po) > MAX_INSTANTS:
        raise ValueError("a trajectory has at most 2^20 instants, got %d" % len(po))
    for Rn, cn in (('R0', 'c0'), ('R1', 'c1')):
        R, c = po[Rn].reshape(po.shape + (3, 3)), po[cn]
        fin = np.isfinite(R).all(axis=(-1, -2)) & np.isfinite(c).all(axis=-1)
        if not fin.all():
            raise ValueError("pose %s, %s and %s must be finite" % (tuple(int(v) for v in np.argwhere(~fin)[0]), Rn, cn))
        off = np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max(axis=(-1, -2))
        bad = (off > POSE_TOL) | (np.abs(np.linalg.det(R) - 1.0) > POSE_TOL)
        if bad.any():
            raise ValueError("pose %s, %s is not orthonormal with determinant +1 (within %g)" %
                             (tuple(int(v) for v in np.argwhere(bad)[0]), Rn, POSE_TOL))
        far = np.sqrt((c * c).sum(axis=-1)) > MAX_CENTRE
        if far.any():
            raise ValueError("pose %s, |%s| is beyond %g m" % (tuple(int(v) for v in np.argwhere(far)[0]), cn, MAX_CENTRE))
    return po
