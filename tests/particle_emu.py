"""The one binding of tests/hostemu/libparticlesemu.so (particles_emu.cpp: the g++ build of what the device particle kernels chain)
and the one "g++ == numpy" comparison of the tests/test_particle_*_host.py.  A frame's settings travel as one struct with named
fields; the arrays an entry point takes are typed by dtype and rank, so a transposed pair is an error and not a wrong comparison."""
import ctypes
import os

import numpy as np

import helpers as h

_V, _I, _U32, _D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_double


class ParticleRun(ctypes.Structure):
    """rr_emu_particle_run of particles_emu.cpp, field for field."""
    _fields_ = [('sim', _V), ('cam_hz', _D), ('model', _I), ('counter', _I), ('jitter_deg', _D), ('wx', _D), ('wz', _D),
                ('gust_n', _I), ('gust_frame0', _U32), ('gust_disp', _V), ('rate_n', _I), ('rate_frame0', _U32), ('rate_dlam', _V),
                ('view', _V), ('pose', _V), ('box', _V), ('dgrid', _V), ('cdf', _V), ('n_grid', _I)]


def _arr(dtype, ndim=1):
    return np.ctypeslib.ndpointer(dtype=dtype, ndim=ndim, flags='C_CONTIGUOUS')


_F64, _RUN = _arr(np.float64), ctypes.POINTER(ParticleRun)
_lib = None


def load():
    """The library, opened once (build() has made it: the `built` fixture): the struct's size checked against the C side, every
    entry point's argtypes and restype set."""
    global _lib
    if _lib is None:
        lib = ctypes.CDLL(os.path.join(h.ROOT, 'tests', 'hostemu', 'libparticlesemu.so'))
        lib.rr_emu_sizeof_particle_run.restype = _I
        assert lib.rr_emu_sizeof_particle_run() == ctypes.sizeof(ParticleRun), (lib.rr_emu_sizeof_particle_run(), ctypes.sizeof(ParticleRun))
        drops = _arr(h.hb.DROP_DTYPE)
        for name, res, args in (
                ('rr_emu_particles', _I, [_RUN, _arr(np.float64, 2), _arr(np.uint8), _F64, _arr(np.int32)]),
                ('rr_emu_records', _I, [_RUN, _I, _I, _F64, drops, _F64, _I]),
                ('rr_emu_jitter_deviates', None, [_V, _I, _arr(np.uint32), _V, _F64]),
                ('rr_emu_sizeof_traj_pose', _I, []),
                ('rr_emu_det_log', None, [ctypes.c_int64, _F64, _F64]),
                ('rr_emu_polar_factor', None, [ctypes.c_int64, _F64, _F64]),
                ('rr_emu_det_sincos', None, [ctypes.c_int64, _F64, _F64, _F64]),
                ('rr_emu_noise_rotate', None, [ctypes.c_int64, drops, _F64, _D, _D]),
                ('rr_emu_drop_in_frame', ctypes.c_int, [_V, _I, _I])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def run(*, model, sim, dgrid, cdf, cam_hz=0.0, view=None, pose=None, box=None, counter=False, jitter=0.0, wind=(0.0, 0.0), gusts=None,
        rate_series=None):
    """The settings of one frame.  model: 'iid' | 'field' | 'rig'; sim: the frame's one rr_sim_frame record; view / pose: the one
    rr_rig_view / rr_traj_pose record of the rig at rest / under a trajectory; gusts / rate_series: tools/particles.py GustSeries /
    RateSeries or None.  The struct keeps the arrays it points to alive."""
    r = ParticleRun(cam_hz=float(cam_hz), model=h.hb.PARTICLE_MODELS[model], counter=int(bool(counter)), jitter_deg=float(jitter),
                    wx=float(wind[0]), wz=float(wind[1]), n_grid=len(dgrid))
    keep = dict(sim=np.ascontiguousarray(sim), dgrid=np.ascontiguousarray(dgrid, np.float64), cdf=np.ascontiguousarray(cdf, np.float64))
    assert keep['sim'].shape == (1,) and keep['cdf'].shape == keep['dgrid'].shape
    for name, a, dtype in (('view', view, h.hb.RIG_VIEW_DTYPE), ('pose', pose, h.hb.TRAJ_POSE_DTYPE), ('box', box, np.float64)):
        if a is not None:
            keep[name] = np.ascontiguousarray(a, dtype)
            assert keep[name].shape == ((3,) if name == 'box' else (1,)), (name, keep[name].shape)
    if gusts is not None:
        r.gust_n, r.gust_frame0 = gusts.n, gusts.frame0
        keep['gust_disp'] = np.ascontiguousarray(gusts.disp, np.float64)
    if rate_series is not None:
        r.rate_n, r.rate_frame0 = rate_series.n, rate_series.frame0
        keep['rate_dlam'] = np.ascontiguousarray(rate_series.dlam(), np.float64)
    for name, a in keep.items():
        setattr(r, name, a.ctypes.data)
    r.arrays = keep
    return r


def all_slots(r):
    """Every particle / slot of the frame, kept or not: (13 columns, inside, life, texture pick)."""
    n = int(r.arrays['sim'][0]['n_particles'])
    out13, inside, life, pick = np.zeros((n, 13)), np.zeros(n, np.uint8), np.zeros(n), np.full(n, -1, np.int32)
    assert load().rr_emu_particles(ctypes.byref(r), out13, inside, life, pick) == 0, 'refused'
    return out13, inside, life, pick


def records(r, H, W, ratio_db):
    """The frame's finished records and the jitter's deviate of each (0 for Big drops and without jitter)."""
    n = int(r.arrays['sim'][0]['n_particles'])
    out, g = np.zeros(n, h.hb.DROP_DTYPE), np.zeros(n)
    m = load().rr_emu_records(ctypes.byref(r), H, W, np.ascontiguousarray(ratio_db, np.float64), out, g, n)
    assert 0 <= m <= n, 'refused' if m < 0 else m
    return out[:m], g[:m]


def assert_slots_equal(out13, life, rec, rec_life, what):
    """all_slots' columns and lives against the numpy statement's particles (cull off), bit for bit."""
    for name, cols in (('wp1', slice(0, 3)), ('wp2', slice(3, 6)), ('ip1', slice(7, 9)), ('ip2', slice(9, 11))):
        assert out13[:, cols].tobytes() == np.ascontiguousarray(rec[name]).tobytes(), (name, what)
    assert out13[:, 6].tobytes() == rec['wd1'].tobytes() and out13[:, 11].tobytes() == rec['iw1'].tobytes(), what
    assert out13[:, 12].tobytes() == rec['iw2'].tobytes() and life.tobytes() == np.ascontiguousarray(rec_life).tobytes(), what


def _bytes_equal(a, b):
    return a.tobytes() == b.tobytes()


def assert_records_equal(got, want, draws, what, same_field=_bytes_equal):
    """records() against expected_records, field by field.  draws == 'stream': the particle kernel leaves the first texture of the
    block of ten to k_particle_draws, which picks one of the ten.  same_field: the comparison of every other field."""
    assert len(got) == len(want), (what, len(got), len(want))
    for name in h.hb.DROP_DTYPE.names:
        if name == 'tex_index' and draws == 'stream':
            assert np.array_equal(got[name], want[name] // 10 * 10), (what, name)
        else:
            assert same_field(got[name], want[name]), (what, name)
