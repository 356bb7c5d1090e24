"""CPU tier: gusts -- a wind that changes over time in the field and rig models (tools/particles.py gusts=, rr_particles.h GUST,
rr_set_particle_gusts).  The series is the air's displacement G[0 .. n] sampled at frame times; a drop born `back` frames ago has
been carried by dG = G[m] - G(m - back) and its streak ends with the frame's air velocity ge = (G[m + 1] - G[m]) cam_hz.

  1. the g++ build of the RR_HD statement (tests/hostemu/particles_emu.cpp: the code the GUST kernels run) == numpy, bit for bit, for
     every slot kept or culled and for the finished records: field, rig (stereo, a yaw ring), a trajectory that yaws and pitches;
     both draws, jitter 0 / 5, mean wind (0, 0) / (-7.5, 2); series with n = 1, a frame at m = 0, frame0 = 2^31 + 3, a frame at m = n - 1;
  2. gusts=None gives the bytes of the functions called without the keyword, also at wind_sigma = 0;
  3. an all-zero series gives the mean wind's records in value;
  4. a constant-velocity series is a mean wind, within a bound from the operation count;
  5. tracks move with the air, streaks are (v + ge) exposure, the slant follows ge and flips in a view yawed by 180 degrees;
  6. a field frame under a sigma = 4 m/s series follows the i.i.d. model's law;
  7. gust_series: reproducible, the right variance, a sequential sum;
  8. every refusal."""
import importlib
import os

import numpy as np
import pytest

import helpers as h
import particle_cases as cases
import particle_emu as pe

particles = importlib.import_module('rain-rendering_amd.tools.particles')
U = cases.U
HZ, BIG0 = cases.HZ, cases.BIG0
WINDS = [(0.0, 0.0), (-7.5, 2.0)]
# (name, model, rig, trajectory)
CASES = [c for c in cases.CASES if c[1] != 'iid']
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope='module')
def emu(built):
    return pe.load()


@pytest.fixture(scope='module')
def sdb(tmp_path_factory):
    return h.Scene(tmp_path_factory.mktemp('gusts'), 64, 96, 10).db     # (only the texture ratios are used)


def _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, view, box, **kw):
    """Every slot of record `s` (cull off): (records, life) of the numpy statement."""
    n, k = int(s['n_particles']), int(s['frame'])
    seed = int(s['key0']) | (int(s['key1']) << 32)
    if model == 'field':
        return particles.make_field_particles(cam, dgrid, tab, n, k, seed, hz, cull=False, **kw)
    if traj is None:
        return particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, rig.views[view], tuple(box), cull=False, **kw)
    po = traj.compose(rig, cam.exposure)[k, view]
    return particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, (po['R0'], po['c0']), tuple(box), cull=False,
                                        view_end=(po['R1'], po['c1']), **kw)


# ---- 1. g++ == numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
def test_gxx_build_equals_numpy(emu, sdb, name, model, rig, traj):
    total = n_before = 0
    for gusts, frames in cases.gust_cases(traj is not None):
        opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, frames)
        hz = float(opt['cam_hz'])
        assert hz == HZ
        V = len(rig) if rig is not None else 1
        W, H = opt["cam_CCD_WH"]
        ratio_db = np.ascontiguousarray(np.asarray(sdb.ratio, np.float64)[:4])
        tab = np.ascontiguousarray(cdf[0])
        views = rig.as_records() if rig is not None else None
        poses = traj.compose(rig, cam.exposure) if traj is not None else None
        for wind in WINDS:
            mean_only = particles.expected_records(sims, dgrid, cdf, sdb, wind=wind, **kw)
            want = {(d, j): particles.expected_records(sims, dgrid, cdf, sdb, draws=d, jitter=j, wind=wind, gusts=gusts, **kw)
                    for d in ('counter', 'stream') for j in (0.0, 5.0)}
            for i, s in enumerate(sims):
                v = i % V
                view = views[v:v + 1] if views is not None and traj is None else None
                po = poses[int(s['frame']), v:v + 1] if traj is not None else None
                air = dict(model=model, sim=sims[i:i + 1], cam_hz=hz, view=view, pose=po, box=box, dgrid=dgrid, cdf=tab, wind=wind, gusts=gusts)
                rec, life = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, v, box, wind=wind, gusts=gusts)
                out, ins, lf, _ = pe.all_slots(pe.run(**air))
                pe.assert_slots_equal(out, lf, rec, life, (i, wind, frames))
                for (draws, jit), recs in want.items():
                    got, _ = pe.records(pe.run(counter=draws == 'counter', jitter=jit, **air), H, W, ratio_db)
                    m, w = len(got), recs[i]
                    assert m == len(w) > 100, (i, wind, draws, jit, m, len(w))
                    pe.assert_records_equal(got, w, draws, (i, wind, draws, jit), cases._same_field)
                    total += m
                assert want[('stream', 0.0)][i].tobytes() != mean_only[i].tobytes()     # the series does something
        # the branch sb < 0 is reached where the frame is the series' first
        if int(sims[0]['frame']) == gusts.frame0:
            s = sims[0]
            seed = int(s['key0']) | (int(s['key1']) << 32)
            j = np.arange(int(s['n_particles']), dtype=np.uint64)
            D, phase, _, z_max = particles._slot_draw(cam, dgrid, tab, j, particles._key(seed), 1.0, 15.0)
            wy = 2.0 * (box[1] * z_max + box[2]) if rig is not None else 2.0 * ((((0.5 + 0.05) * float(cam.H)) / cam.fpx) * z_max)
            tau = particles._slot_fall(cam, hz, int(s['frame']), j, particles._key(seed), D, wy, phase, 1.0)[3]
            n_before += int((tau * hz > 0).sum())
    assert n_before > 100
    print('%s: %d records compared, %d births before a series' % (name, total, n_before))


# ---- 2. off == today -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("wind_sigma", [1.0, 0.0])
def test_no_series_gives_the_bytes_without_the_keyword(sdb, name, model, rig, traj, wind_sigma):
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, [0, 1])
    sims['wind_sigma'] = wind_sigma
    hz = float(opt['cam_hz'])
    for wind in WINDS:
        for draws, jit in (('stream', 0.0), ('counter', 5.0)):
            a = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, wind=wind, **kw)
            b = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, wind=wind, gusts=None, **kw)
            assert all(len(x) > 100 and x.tobytes() == y.tobytes() for x, y in zip(a, b))
        V = len(rig) if rig is not None else 1
        tab = np.ascontiguousarray(cdf[0])
        for i, s in enumerate(sims):
            a = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, i % V, box, wind=wind, wind_sigma=wind_sigma)
            b = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, i % V, box, wind=wind, wind_sigma=wind_sigma, gusts=None)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            if model == 'rig':
                n, k = int(s['n_particles']), int(s['frame'])
                seed = int(s['key0']) | (int(s['key1']) << 32)
                sa = particles.rig_state(cam, dgrid, tab, n, k, seed, hz, tuple(box), wind_sigma=wind_sigma, wind=wind)
                sb = particles.rig_state(cam, dgrid, tab, n, k, seed, hz, tuple(box), wind_sigma=wind_sigma, wind=wind, gusts=None)
                assert all(sa[key].tobytes() == sb[key].tobytes() for key in sa)
    opt2 = cases.options('kitti')
    if model == 'field':
        a, b = particles.generate(opt2, 25, 2, seed=3, model='field'), particles.generate(opt2, 25, 2, seed=3, model='field', gusts=None)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        fa, fb = particles.field_frame(opt2, 25, 4, seed=3), particles.field_frame(opt2, 25, 4, seed=3, gusts=None)
        assert fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes()
        ka = particles.field_kinematics(cam, dgrid, cdf[0], fa[0]['pid'], fa[1], 3)
        kb = particles.field_kinematics(cam, dgrid, cdf[0], fa[0]['pid'], fa[1], 3, gusts=None)
        assert ka[0].tobytes() == kb[0].tobytes() and ka[1].tobytes() == kb[1].tobytes()
    else:
        a = particles.rig_frame(opt2, 25, 1, rig, 0, seed=3, trajectory=traj)
        b = particles.rig_frame(opt2, 25, 1, rig, 0, seed=3, trajectory=traj, gusts=None)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 3. a zero series is the mean wind -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
def test_a_zero_series_is_the_mean_wind(sdb, name, model, rig, traj):
    """dG = 0 - (0 + fr (0 - 0)) and ge = (0 - 0) cam_hz are zeros: x + 0 == x in value (only a zero's sign may differ)."""
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, [0, 2])
    zero = particles.GustSeries(0, np.zeros((4, 2)))
    for wind in [(-7.5, 2.0), (3.0, 0.0)]:
        for draws, jit in (('stream', 0.0), ('counter', 5.0)):
            a = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, wind=wind, **kw)
            b = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, wind=wind, gusts=zero, **kw)
            for x, y in zip(a, b):
                assert len(x) == len(y) > 100
                for nm in h.hb.DROP_DTYPE.names:
                    assert np.array_equal(x[nm], y[nm], equal_nan=x[nm].dtype.kind == 'f'), (wind, draws, jit, nm)


# ---- 4. a constant-velocity series is a mean wind ------------------------------------------------------------------
STEP = 0.25                                               # metres per frame at 10 Hz: 2.5 m/s along x
N_CONST = 40


def _const_series():
    d = np.zeros((N_CONST + 1, 2))
    d[:, 0] = np.arange(N_CONST + 1) * STEP
    return particles.GustSeries(0, d)


def _const_bounds(vx, vxm, tau, m, w, q, X, e):
    """|position difference| and |end difference| along x between the gust path under G[i] = 0.25 i and the mean-wind path under
    wx + 2.5, u = 2^-53, from the operation count.
      dG: back = fl(tau hz) (u back), sb = fl(m - back) (u max(m, back) =: u M), fr = sb - i exact, G[i + 1] - G[i] = 0.25 exact,
        fr 0.25 exact, Gb = fl(G[i] + .) (u |Gb| <= u 0.25 M), dG = fl(G[m] - Gb) (u |dG| <= u 0.25 (M + back)); the exact value
        is 0.25 back = 2.5 tau: |dG - 2.5 tau| <= E_dG = 4 u 0.25 (M + back).
      S_g = fl(fl(vx tau) + dG), S_m = fl(vx' tau) with vx = fl(wl + wx), vx' = fl(wl + wx + 2.5) (wx + 2.5 is exact for the winds
        used): |vx' - (vx + 2.5)| <= u (|vx| + |vx'|); |S_g - S_m| <= E_S = E_dG + u |vx tau| + u |S_g| + u |S_m| + tau u (|vx| + |vx'|).
      q = fl(u32 + fl(S / w)) on either side: |q_g - q_m| <= E_S / w + 2 u |S| / w + 2 u |q|; f = q - floor(q) is exact (the same
        floor: slots within 1e-9 of an integer are left out); X = fl(fl(f w) - bx): 2 u (w + |X|) for the two sides.
      end = fl(X + fl(ve e)), ve = fl(vx + 2.5) against vx': e u (|vx| + 2 |vx'|) + 2 u |ve e| + 2 u |X2| more.
    Every |.| is taken with (1 + 2^-20) for the second-order terms."""
    back = tau * HZ
    M = np.maximum(float(m), back)
    E_dG = 4.0 * U * STEP * (M + back)
    S = np.abs(vxm * tau)
    E_S = E_dG + U * np.abs(vx * tau) + 2.0 * U * S + tau * U * (np.abs(vx) + np.abs(vxm))
    pos = (E_S + 2.0 * U * S + 2.0 * U * np.abs(q) * w + 2.0 * U * (w + np.abs(X))) * (1.0 + 2.0 ** -20)
    end = pos + (e * U * (np.abs(vx) + 2.0 * np.abs(vxm)) + 2.0 * U * np.abs(vxm * e) + 2.0 * U * (np.abs(X) + np.abs(vxm * e))) * (1.0 + 2.0 ** -20)
    return pos, end


@pytest.mark.parametrize("model", ['field', 'rig'])
@pytest.mark.parametrize("wind", WINDS)
def test_a_constant_velocity_series_is_a_mean_wind(model, wind):
    gusts = _const_series()
    rig = cases.KITTI_STEREO if model == 'rig' else None
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, None, [0])
    tab = np.ascontiguousarray(cdf[0])
    n = int(sims[0]['n_particles'])
    seed = cases.SEED
    key = particles._key(seed)
    j = np.arange(n, dtype=np.uint64)
    windm = (wind[0] + 2.5, wind[1])
    left_out = total = 0
    for k in (0, 17, N_CONST - 1):                           # births before the series, inside it, its last frame
        D, phase, wd, z_max = particles._slot_draw(cam, dgrid, tab, j, key, 1.0, 15.0)
        if model == 'field':
            hy = ((0.5 + 0.05) * float(cam.H)) / cam.fpx
            w, wy = 2.0 * ((((0.5 + 0.05) * float(cam.W)) / cam.fpx) * z_max), 2.0 * (hy * z_max)
            zdiv, zsign = z_max, -1.0
        else:
            w, wy = 2.0 * (box[0] * z_max), 2.0 * (box[1] * z_max + box[2])
            zdiv, zsign = w, 1.0
        v, g, age, tau, b, wl = particles._slot_fall(cam, HZ, k, j, key, D, wy, phase, 1.0)
        vx, vz = particles._drift(wl, cam.speed, wind, gusts)
        vxm, _ = particles._drift(wl, cam.speed, windm)
        qx = particles.unit32(b[0]) + (vxm * tau) / w
        qz = particles.unit32(b[1]) + zsign * ((vz * tau) / zdiv)
        near = (np.abs(qx - np.rint(qx)) < 1e-9) | (np.abs(qz - np.rint(qz)) < 1e-9)
        if model == 'field':
            a, la = particles.make_field_particles(cam, dgrid, tab, n, k, seed, HZ, cull=False, wind=wind, gusts=gusts)
            c, lc = particles.make_field_particles(cam, dgrid, tab, n, k, seed, HZ, cull=False, wind=windm)
            pa, pc, ea, ec = a['wp1'], c['wp1'], a['wp2'], c['wp2']
            ok = ~near                                            # (a clamped depth is clamped alike on both sides: z does not see the series)
        else:
            sa = particles.rig_state(cam, dgrid, tab, n, k, seed, HZ, tuple(box), wind=wind, gusts=gusts)
            sc = particles.rig_state(cam, dgrid, tab, n, k, seed, HZ, tuple(box), wind=windm)
            la, lc = sa['life'], sc['life']
            pa, pc = sa['pos'], sc['pos']
            ea, ec = sa['pos'] + sa['vel'] * cam.exposure, sc['pos'] + sc['vel'] * cam.exposure
            ok = ~near
        assert np.array_equal(la, lc)
        pos, end = _const_bounds(vx, vxm, tau, k, w, qx, pc[:, 0], cam.exposure)
        if model == 'rig':                                        # the end is formed here: one product and one sum more on either side
            end = end + 4.0 * U * (np.abs(pc[:, 0]) + np.abs(vxm * cam.exposure))
        # y and z do not see the series: the z column of G is zero, so dGz and gez are zeros
        assert np.array_equal(pa[ok][:, 1:], pc[ok][:, 1:]) and np.array_equal(ea[ok][:, 1], ec[ok][:, 1])
        assert np.all(np.abs(ea[ok][:, 2] - ec[ok][:, 2]) <= 4.0 * U * (np.abs(ec[ok][:, 2]) + 1.0))
        dp, de = np.abs(pa[:, 0] - pc[:, 0])[ok], np.abs(ea[:, 0] - ec[:, 0])[ok]
        print('%s wind %s frame %d: %d slots, %d left out, worst |d| / bound: position %.3f, end %.3f'
              % (model, wind, k, int(ok.sum()), int((~ok).sum()), (dp / pos[ok]).max(), (de / end[ok]).max()))
        assert np.all(dp <= pos[ok]) and np.all(de <= end[ok])
        left_out += int(near.sum())
        total += n
    assert left_out * 1000 <= total, (left_out, total)


# ---- 5. tracks move with the air -----------------------------------------------------------------------------------
def _gust_err(gusts, back, m):
    """The rounding of dG per component, u = 2^-53: back = fl(tau hz) and sb = fl(m - back) move the birth by u (back + max(m, back))
    frames, i.e. by that times the largest |step|; G[i + 1] - G[i], its product with the fraction (< 1), the sum Gb and the
    difference dG one rounding each of values <= max |step|, max |step|, max |G|, 2 max |G|."""
    smax = np.abs(np.diff(gusts.disp, axis=0)).max()
    gmax = np.abs(gusts.disp).max()
    return U * (smax * (back + np.maximum(m, back) + 2.0) + 3.0 * gmax)


def test_field_tracks_move_with_the_air():
    """A slot kept at k and k + 1 in one life: wp1(k + 1) - wp1(k) = (vx, -v, vz) / cam_hz + (G[m + 1] - G[m]) modulo the box.  The
    birth instant is the same in both frames, so Gb cancels in exact arithmetic.  Bound: the wind's own (cases._windy_bounds over
    cases._track_bounds) taken with |velocity| + max |step| cam_hz on x and z -- the error of tau moves the birth, and the air is never
    faster than that --, plus _gust_err for each of the two frames, plus 2 u |G[m + 1] - G[m]| for the difference formed here."""
    wind = (-7.5, 2.0)
    gusts = particles.gust_series(12, HZ, 4.0, 2.0, seed=21, frame0=1000)
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([50.0])})
    cam = particles.FrameCamera(opt, 0)
    _, dgrid, cdf, _ = particles.expected_count(cam, 25)
    dt = 1.0 / cam.hz
    smax = np.abs(np.diff(gusts.disp, axis=0)).max()
    total = 0
    for k in range(1000, 1011):
        m = k - gusts.frame0
        ra, la = particles.field_frame(opt, 25, k, seed=11, wind=wind, gusts=gusts)
        rb, lb = particles.field_frame(opt, 25, k + 1, seed=11, wind=wind, gusts=gusts)
        _, ia, ib = np.intersect1d(ra['pid'], rb['pid'], return_indices=True)
        ok = (la[ia] == lb[ib]) & (ra['wp1'][ia, 2] < -0.05) & (rb['wp1'][ib, 2] < -0.05)
        ia, ib = ia[ok], ib[ok]
        if len(ia) == 0:
            continue
        vel, box = particles.field_kinematics(cam, dgrid, cdf, ra['pid'][ia], la[ia], 11, wind=wind, gusts=gusts)
        step = gusts.disp[m + 1] - gusts.disp[m]
        want = vel * dt
        want[:, 0] += step[0]
        want[:, 2] += step[1]                                     # (air moving toward the viewer shrinks the depth: wp1's z = -depth grows)
        r = (rb['wp1'][ib] - ra['wp1'][ia]) - want
        r[:, 0] -= box[:, 0] * np.rint(r[:, 0] / box[:, 0])
        r[:, 2] -= box[:, 2] * np.rint(r[:, 2] / box[:, 2])
        veff = vel.copy()
        veff[:, 0] = np.abs(vel[:, 0]) + smax * HZ
        veff[:, 2] = np.abs(vel[:, 2]) + smax * HZ
        bound = cases._windy_bounds(cases._track_bounds(veff, box, la[ia], dt), veff, box, la[ia], dt)
        T = box[:, 1] / np.abs(vel[:, 1])
        ge = 2.0 * _gust_err(gusts, T * HZ + 1.0, float(m + 1)) + 2.0 * U * np.abs(step).max()
        bound[:, 0] += ge
        bound[:, 2] += ge
        print('frame %d -> %d: %d kept again, worst |residual| / bound per axis %s' % (k, k + 1, len(ia), (np.abs(r) / bound).max(axis=0)))
        assert np.all(np.abs(r) <= bound), (np.abs(r) / bound).max(axis=0)
        # and the air's step is what the test sees: without it the residual is the step itself
        if np.abs(step[0]) > 1e-3:
            r0 = (rb['wp1'][ib, 0] - ra['wp1'][ia, 0]) - vel[:, 0] * dt
            r0 -= box[:, 0] * np.rint(r0 / box[:, 0])
            assert np.all(np.abs(r0 - step[0]) <= bound[:, 0]) and np.all(np.abs(r0) > bound[:, 0])
        total += len(ia)
    assert total >= 60, total


@pytest.mark.parametrize("name,model,rig", [('field', 'field', None), ('rig-ring', 'rig', cases.RING3)])
def test_a_streak_is_the_velocity_with_the_gust_times_the_exposure(sdb, name, model, rig):
    """Every kept record: wpe - wps = R (vx + gex, -v(D), vz + gez) exposure in the view's axes, within the mean wind's bound
    (tests/test_particle_wind_host.py) with one more rounding of the velocity: vx + gex is a rounded sum, formed here with the same
    bits, and ge itself -- a difference of two table entries times cam_hz -- is formed here with the same two operations."""
    wind = (-7.5, 2.0)
    gusts, frames = cases.gust_cases()[1]
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, None, frames)
    hz = float(opt['cam_hz'])
    tab = np.ascontiguousarray(cdf[0])
    recs = particles.expected_records(sims, dgrid, cdf, sdb, wind=wind, gusts=gusts, **kw)
    V = len(rig) if rig is not None else 1
    for i, s in enumerate(sims):
        table, _, W, H = particles._loaded_table(s, dgrid, cdf, sdb, 'kitti', model, hz, rig, i % V, wind=wind, gusts=gusts)
        pid = table.pid[h.hb.filter_streaks(table, W, H)]
        rec = recs[i]
        assert len(pid) == len(rec) > 100
        allp, life = _all_slots(model, cam, dgrid, tab, s, hz, rig, None, i % V, box, wind=wind, gusts=gusts)
        v = particles.terminal_velocity(allp['wd1'][pid] * 1e3)
        seed = int(s['key0']) | (int(s['key1']) << 32)
        own = particles._block_wind(particles.philox4x32(*particles._life_counter(pid.astype(np.uint64), life[pid], 2), *particles._key(seed)), 1.0)
        m = int(s['frame']) - gusts.frame0
        ge = (gusts.disp[m + 1] - gusts.disp[m]) * hz
        assert np.abs(ge).max() > 0.1
        vel = np.stack([(own + wind[0]) + ge[0], -v, np.full(len(pid), (cam.speed + wind[1]) + ge[1])], axis=1)
        R = np.eye(3) if rig is None else np.asarray(rig.views[i % V][0], np.float64).reshape(3, 3)
        want = (vel * cam.exposure) @ R.T
        want[:, 2] = -want[:, 2]                                   # the record's z is the depth
        got = rec['wpe'] - rec['wps']
        free = rec['wps'][:, 2] > 0.05
        if rig is None:
            bound = U * (np.abs(rec['wpe']) + np.abs(got)) + 2.0 * U * np.abs(want)
        else:
            bound = (10.0 * U * (np.sqrt((rec['wps'] ** 2).sum(axis=1)) + np.sqrt((want ** 2).sum(axis=1))))[:, None] * np.ones(3)
        bound[:, 1] += 4.0 * U * np.abs(want[:, 1])                # v(D) of the D read back from the record's diameter in metres
        err = np.abs(got - want)[free]
        print('%s record %d: worst |error| / bound per axis %s' % (name, i, (err / bound[free]).max(axis=0)))
        assert np.all(err <= bound[free]), (err / bound[free]).max(axis=0)
        assert free.sum() > 100


def _slant_series():
    """Two frames whose air velocity differs: +6 m/s along x over the first interval, -6 m/s over the second."""
    return particles.GustSeries(0, np.array([[0.0, 0.0], [0.6, 0.0], [0.0, 0.0]]))


def test_the_slant_follows_the_gust_and_flips_in_a_view_yawed_180_degrees(sdb):
    """No scatter, no ego-motion, no mean wind: the projected streak is (gex, v) e fpx / depth, dx / dy = gex / v(D) up to the two
    end points' rounding to pixels (half a pixel each: |dx - r dy| <= 1 + |r|).  Frame 0 leans right, frame 1 left; the view that
    looks backwards sees the opposite in both."""
    gusts = _slant_series()
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run('rig', cases.BACK_TO_BACK, None, [0, 1], speed_kmh=0.0)
    sims['wind_sigma'] = 0.0
    recs = particles.expected_records(sims, dgrid, cdf, sdb, gusts=gusts, **kw)
    hz = float(opt['cam_hz'])
    for i, rec in enumerate(recs):
        frame, view = i // 2, i % 2
        gex = (gusts.disp[frame + 1, 0] - gusts.disp[frame, 0]) * hz
        sign = (1.0 if view == 0 else -1.0) * np.sign(gex)
        table, _, W, H = particles._loaded_table(sims[i], dgrid, cdf, sdb, 'kitti', 'rig', hz, cases.BACK_TO_BACK, view, gusts=gusts)
        pid = table.pid[h.hb.filter_streaks(table, W, H)]
        D = particles._slot_draw(cam, dgrid, cdf[0], pid.astype(np.uint64), particles._key(cases.SEED), 1.0, 15.0)[0]
        r = sign * abs(gex) / particles.terminal_velocity(D)
        dx, dy = (rec['x1'] - rec['x0']).astype(np.float64), (rec['y1'] - rec['y0']).astype(np.float64)
        nb = rec['type'] != 0
        assert nb.sum() > 100 and np.all(sign * dx >= 0) and (sign * dx[nb]).max() >= 3
        assert np.all(np.abs(dx - r * dy)[nb] <= (1.0 + np.abs(r[nb])) * (1.0 + 1e-12))


# ---- 6. the law ----------------------------------------------------------------------------------------------------
def test_a_gusty_field_frame_has_the_iid_models_law():
    opt = cases.options('kitti')
    cam = particles.FrameCamera(opt, 0)
    gusts = particles.gust_series(7 * cases.N_LAW + 4, HZ, 4.0, 2.0, seed=77)
    counts, D, depth, px, py = [], [], [], [], []
    for i in range(cases.N_LAW):                                  # cases._sample('field', 9000) under the series
        rec, _ = particles.field_frame(opt, 25, 7 * i + 3, seed=9000 + i, gusts=gusts)
        counts.append(len(rec))
        D.append(rec['wd1'] * 1e3)
        depth.append(-rec['wp1'][:, 2])
        px.append(rec['ip1'][:, 0])
        py.append(rec['ip1'][:, 1])
    field = dict(cam=cam, counts=np.array(counts), D=np.concatenate(D), depth=np.concatenate(depth), px=np.concatenate(px), py=np.concatenate(py))
    iid_a, iid_b = cases._sample('iid', 1000), cases._sample('iid', 5000)
    control = cases._same_law(iid_a, iid_b)
    assert all(v < 1 for v in control.values()), control
    mean = particles.expected_count(cam, 25)[0]
    assert abs(field['counts'].mean() - mean) < 4 * np.sqrt(mean / cases.N_LAW)
    got, got_b = cases._same_law(field, iid_a), cases._same_law(field, iid_b)
    print('statistic / threshold -- iid vs iid: %s\n  gusty field vs iid: %s\n  gusty field vs iid (other seeds): %s' % (control, got, got_b))
    assert all(v < 1 for v in got.values()), got
    assert all(v < 1 for v in got_b.values()), got_b
    calm, _ = particles.field_frame(opt, 25, 3, seed=9000)
    gusty, _ = particles.field_frame(opt, 25, 3, seed=9000, gusts=gusts)
    assert calm['pid'].tobytes() != gusty['pid'].tobytes()


# ---- 7. gust_series ------------------------------------------------------------------------------------------------
def test_gust_series():
    a, b, c = (particles.gust_series(500, HZ, 3.0, 2.0, seed=s) for s in (4, 4, 5))
    assert a.disp.tobytes() == b.disp.tobytes() != c.disp.tobytes() and a.frame0 == 0 and a.n == 500 and a.disp.shape == (501, 2)
    assert particles.gust_series(3, HZ, 3.0, 2.0, seed=4, frame0=BIG0).frame0 == BIG0
    # the displacement is the sequential sum of the interval velocities / cam_hz from zero
    rs = np.random.RandomState(4)
    z = rs.standard_normal((500, 2))
    al = float(np.exp(-1.0 / (HZ * 2.0)))
    u = np.zeros((500, 2))
    u[0] = 3.0 * z[0]
    for i in range(1, 500):
        u[i] = al * u[i - 1] + (3.0 * float(np.sqrt(1.0 - al * al))) * z[i]
    acc = np.zeros(2)
    for i in range(500):
        acc = acc + u[i] / HZ
        assert a.disp[i + 1].tobytes() == acc.tobytes()
    assert a.disp[0].tobytes() == np.zeros(2).tobytes()
    # the variance: n correlated normal values per component, corr(u_i, u_j) = a^|i - j|, so corr(u_i^2, u_j^2) = a^(2 |i - j|) and the
    # variance of the mean of squares (known zero mean) is (2 sigma^4 / N) (1 + a^2) / (1 - a^2) for the N = 2 n pooled values
    n, sigma, tau_s = 20000, 4.0, 0.05
    g = particles.gust_series(n, HZ, sigma, tau_s, seed=1)
    vel = np.diff(g.disp, axis=0) * HZ
    al = np.exp(-1.0 / (HZ * tau_s))
    se = sigma ** 2 * np.sqrt(2.0 / (2 * n) * (1 + al ** 2) / (1 - al ** 2))
    var = (vel ** 2).mean()
    print('sample variance %.4f, sigma^2 %.1f, standard error %.4f' % (var, sigma ** 2, se))
    assert abs(var - sigma ** 2) <= se
    assert abs(vel.mean()) <= 4.0 * sigma * np.sqrt((1 + al) / (1 - al) / (2 * n))
    # the correlation time: lag-one correlation a = exp(-dt / tau)
    g2 = particles.gust_series(20000, HZ, 4.0, 1.0, seed=2)
    v2 = np.diff(g2.disp, axis=0)[:, 0] * HZ
    rho = (v2[1:] * v2[:-1]).mean() / (v2 ** 2).mean()
    assert abs(rho - np.exp(-0.1)) < 0.02
    for bad in (dict(n=0), dict(n=2 ** 20 + 1), dict(sigma=-1.0), dict(tau_s=0.0), dict(cam_hz=0.0), dict(sigma=float('nan'))):
        kw = dict(n=4, cam_hz=HZ, sigma=1.0, tau_s=1.0, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            particles.gust_series(**kw)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(sdb):
    G = particles.GustSeries
    ok = np.array([[0.0, 0.0], [0.1, 0.0], [0.2, 0.1]])
    assert particles._check_gusts(None, None, 'iid') is None
    assert particles._check_gusts(G(0, ok), HZ).n == 2
    particles._check_gusts(G(2 ** 32 - 2, ok), HZ)                                    # frame0 + n = 2^32 is allowed
    particles._check_gusts(G(0, np.array([[0.0, 0.0], [10.0, 0.0]])), HZ)             # 100 m/s itself is allowed
    bad = [G(2 ** 32 - 1, ok), G(-1, ok), G(0, ok[:1]), G(0, np.zeros((3, 3))), G(0, np.zeros(4)),
           G(0, np.array([[0.0, 0.0], [np.nan, 0.0]])), G(0, np.array([[0.0, 0.0], [0.0, np.inf]])),
           G(0, np.array([[1e6, 1.0], [1e6, 1.0]])), G(0, np.array([[0.0, 0.0], [8.0, 8.0]])), (0, ok), 'gusts']
    for g in bad:
        with pytest.raises(ValueError, match='gust'):
            particles._check_gusts(g, HZ)
    with pytest.raises(ValueError, match='2\\^20'):
        particles._check_gusts(G(0, np.zeros((2 ** 20 + 2, 2))), HZ)
    for hz in (None, 0.0, float('nan')):
        with pytest.raises(ValueError, match='cam_hz'):
            particles._check_gusts(G(0, ok), hz)
    with pytest.raises(ValueError, match='no time'):
        particles._check_gusts(G(0, ok), HZ, 'iid')
    # the generator's: the i.i.d. model, a frame outside the series, run_pos
    opt = cases.options('kitti')
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1)
    with pytest.raises(ValueError, match='no time'):
        particles.expected_records(sims, dgrid, cdf, sdb, gusts=G(0, ok))
    with pytest.raises(ValueError, match='no time'):
        particles.generate(opt, 25, 1, gusts=G(0, ok))
    opt, fs, dgrid, cdf, kw, cam, box = cases.case_run('field', None, None, [2])
    with pytest.raises(ValueError, match='outside the gust series'):
        particles.expected_records(fs, dgrid, cdf, sdb, gusts=G(0, ok), **kw)
    with pytest.raises(ValueError, match='outside the gust series'):
        particles.expected_records(fs, dgrid, cdf, sdb, gusts=G(3, ok), **kw)
    assert len(particles.expected_records(fs, dgrid, cdf, sdb, gusts=G(1, ok), **kw)[0]) > 100
    with pytest.raises(ValueError, match='outside the gust series'):
        particles.field_frame(opt, 25, 2, gusts=G(0, ok))
    with pytest.raises(ValueError, match='outside the gust series'):
        particles.rig_frame(opt, 25, 2, cases.MONO, 0, gusts=G(0, ok))
    runp = fs.copy()
    runp['run_pos'] = 1
    with pytest.raises(ValueError, match='run_pos'):
        particles.expected_records(runp, dgrid, cdf, sdb, gusts=G(1, ok), **kw)
    with pytest.raises(ValueError, match='no angular noise'):
        particles.expected_records(fs, dgrid, cdf, sdb, noise_std=2.0, noise_scale=1.0, gusts=G(1, ok), **kw)


def test_the_driver_and_the_augmenter_carry_the_series(tmp_path):
    """--gusts SIGMA[,TAU[,SEED]]: parsed next to --wind, needs the field or rig model, --streak_lean auto follows it; RainAugment.plan
    carries the series and refuses a frame_index outside it."""
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', str(tmp_path), '-i', '25']
    field = ['--device_particles', '--particle_model', 'field']

    def parsed(extra):
        ns = main._wind_and_lean(main._parse(common + extra))
        return ns.gusts, ns.lean
    assert parsed([]) == (None, False) and parsed(field) == (None, False)
    assert parsed(field + ['--gusts', '3']) == ((3.0, 2.0, 0), True)
    assert parsed(field + ['--gusts', '3,0.5']) == ((3.0, 0.5, 0), True)
    assert parsed(field + ['--gusts', '3,2,7', '--streak_lean', 'off']) == ((3.0, 2.0, 7), False)
    for bad in ([], ['--device_particles'], field + ['--gusts=0'], field + ['--gusts=-1'], field + ['--gusts=21'], field + ['--gusts=3,0'],
                field + ['--gusts=3,2,1,4'], field + ['--gusts=a'], field + ['--gusts=3,2,-1'], field + ['--gusts=nan']):
        with pytest.raises(SystemExit, match='--gusts'):
            main._derive(main._parse(common + (bad if any(b.startswith('--gusts') for b in bad) else bad + ['--gusts', '3,2'])))
    augment = importlib.import_module('rain-rendering_amd.augment')
    root = str(tmp_path)
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    kw = dict(streaks_db=os.path.join(root, 'rainstreakdb'), sequence='data_object/training')
    gusts = particles.gust_series(12, HZ, 3.0, 2.0, seed=0)
    aug = augment.RainAugment('kitti', particle_model='field', draws='counter', gusts=gusts, **kw)
    p = aug.plan(25, [4, 11])
    assert p['gusts'] is gusts and p['lean'] is True and p['wind'] == (0.0, 0.0)
    recs = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws=p['draws'],
                                      wind=p['wind'], gusts=p['gusts'])
    plain = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws=p['draws'])
    assert len(recs[0]) > 100 and recs[0].tobytes() != plain[0].tobytes()
    with pytest.raises(ValueError, match='outside the gust series'):
        aug.plan(25, [4, 12])
    assert augment.RainAugment('kitti', particle_model='field', gusts=gusts, lean=False, **kw).lean is False
    aug.set_gusts(None)
    assert aug.lean is False and aug.plan(25, [4, 12])['gusts'] is None
    aug.set_gusts(gusts)
    assert aug.lean is True
    for bad in ('gusts', (0, gusts.disp), particles.GustSeries(0, np.array([[0.0, 0.0], [50.0, 0.0]]))):
        with pytest.raises(ValueError, match='gust'):
            augment.RainAugment('kitti', particle_model='field', gusts=bad, **kw)
    with pytest.raises(ValueError, match='no time'):
        augment.RainAugment('kitti', gusts=gusts, **kw)
