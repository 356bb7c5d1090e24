"""CPU tier: showers -- a rain rate that changes over time in the field and rig models (tools/particles.py rate_series=,
rr_particles.h RATE, rr_set_particle_rate_series).  Slots and tables are the PEAK rate's; a life is kept with the probability
exp(-(Lambda(R) - Lambda(R_peak)) D) of the rate R at its birth, decided by word 3 of the life's Philox block 1.

  1. the g++ build of the RR_HD statement (tests/hostemu/particles_emu.cpp: the code the RATE kernels run) == numpy, bit for bit, for
     every slot kept or culled and for the finished records: field, rig (stereo, a yaw ring), a trajectory; both draws, jitter 0 / 5,
     mean wind (0, 0) / (-7.5, 2), with and without a gust series; series with n = 1, a frame at m = 0, frame0 = 2^31 + 3, a frame
     at m = n - 1, a series that touches rate 0;
  2. rate_series=None gives the bytes of the functions called without the keyword; a series constant at its peak gives the bytes of
     no series;
  3. a series constant at 25 mm/hr under a peak of 100 follows the law of a plain 25 mm/hr field;
  4. a ramp 25 -> 5 keeps or drops a (slot, life) for good, kept tracks move by the velocity, the count follows the rate;
  5. a dry spell empties the field after the longest fall period, and what is left before is older than the spell;
  6. both stereo views keep the same (slot, life) among the slots both see;
  7. shower_series' values, every refusal, the driver's flag and RainAugment.plan."""
import importlib
import os

import numpy as np
import pytest

import helpers as h
import particle_cases as cases
import particle_emu as pe

particles = importlib.import_module('rain-rendering_amd.tools.particles')
HZ, PEAK, BIG0 = cases.HZ, cases.PEAK, cases.BIG0
WINDS = [(0.0, 0.0), (-7.5, 2.0)]
R = particles.RateSeries
# (name, model, rig, trajectory)
CASES = [c for c in cases.CASES if c[1] != 'iid']
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope='module')
def emu(built):
    return pe.load()


@pytest.fixture(scope='module')
def sdb(tmp_path_factory):
    return h.Scene(tmp_path_factory.mktemp('showers'), 64, 96, 10).db     # (only the texture ratios are used)


def _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, view, box, **kw):
    """Every slot of record `s`: (records, life) of the numpy statement with the cull off, and the slots it keeps with it on."""
    n, k = int(s['n_particles']), int(s['frame'])
    seed = int(s['key0']) | (int(s['key1']) << 32)
    if model == 'field':
        make = lambda cull: particles.make_field_particles(cam, dgrid, tab, n, k, seed, hz, cull=cull, **kw)
    elif traj is None:
        make = lambda cull: particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, rig.views[view], tuple(box), cull=cull, **kw)
    else:
        po = traj.compose(rig, cam.exposure)[k, view]
        make = lambda cull: particles.make_rig_particles(cam, dgrid, tab, n, k, seed, hz, (po['R0'], po['c0']), tuple(box), cull=cull,
                                                         view_end=(po['R1'], po['c1']), **kw)
    rec, life = make(False)
    kept = np.zeros(n, np.uint8)
    kept[make(True)[0]['pid']] = 1
    return rec, life, kept


# ---- 1. g++ == numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
def test_gxx_build_equals_numpy(emu, sdb, name, model, rig, traj):
    total = n_before = n_rejected = 0
    for rs, frames in cases.rate_cases(traj is not None):
        opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, frames)
        hz = float(opt['cam_hz'])
        assert hz == HZ
        V = len(rig) if rig is not None else 1
        W, H = opt["cam_CCD_WH"]
        ratio_db = np.ascontiguousarray(np.asarray(sdb.ratio, np.float64)[:4])
        tab = np.ascontiguousarray(cdf[0])
        views = rig.as_records() if rig is not None else None
        poses = traj.compose(rig, cam.exposure) if traj is not None else None
        dlam = np.ascontiguousarray(rs.dlam())
        assert dlam.min() >= 0.0 and dlam.max() <= particles.RATE_DLAM_MAX
        for wind in WINDS:
            for gusts in (None, cases.gusts_over(rs)):
                air = dict(wind=wind, gusts=gusts)
                no_series = particles.expected_records(sims, dgrid, cdf, sdb, **air, **kw)
                want = {(d, j): particles.expected_records(sims, dgrid, cdf, sdb, draws=d, jitter=j, rate_series=rs, **air, **kw)
                        for d in ('counter', 'stream') for j in (0.0, 5.0)}
                for i, s in enumerate(sims):
                    v = i % V
                    view = views[v:v + 1] if views is not None and traj is None else None
                    po = poses[int(s['frame']), v:v + 1] if traj is not None else None
                    under = dict(model=model, sim=sims[i:i + 1], cam_hz=hz, view=view, pose=po, box=box, dgrid=dgrid, cdf=tab, rate_series=rs, **air)
                    rec, life, kept = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, v, box, rate_series=rs, **air)
                    _, _, kept_plain = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, v, box, **air)
                    out, ins, lf, _ = pe.all_slots(pe.run(**under))
                    assert ins.tobytes() == kept.tobytes(), (i, wind, gusts is not None, frames)     # every slot: kept or culled
                    assert np.all(kept <= kept_plain)                                               # the series only removes
                    n_rejected += int((kept_plain & ~kept & 1).sum())
                    pe.assert_slots_equal(out, lf, rec, life, (i, wind, frames))
                    for (draws, jit), recs in want.items():
                        got, _ = pe.records(pe.run(counter=draws == 'counter', jitter=jit, **under), H, W, ratio_db)
                        m, w = len(got), recs[i]
                        assert m == len(w) > 100, (i, wind, draws, jit, m, len(w))
                        pe.assert_records_equal(got, w, draws, (i, wind, draws, jit), cases._same_field)
                        total += m
                    assert len(want[('stream', 0.0)][i]) < len(no_series[i])                  # the series does something
        # the held first value is reached where the frame is the series' first
        if int(sims[0]['frame']) == rs.frame0:
            s = sims[0]
            seed = int(s['key0']) | (int(s['key1']) << 32)
            j = np.arange(int(s['n_particles']), dtype=np.uint64)
            D, phase, _, z_max = particles._slot_draw(cam, dgrid, tab, j, particles._key(seed), 1.0, 15.0)
            wy = 2.0 * (box[1] * z_max + box[2]) if rig is not None else 2.0 * ((((0.5 + 0.05) * float(cam.H)) / cam.fpx) * z_max)
            tau = particles._slot_fall(cam, hz, int(s['frame']), j, particles._key(seed), D, wy, phase, 1.0)[3]
            n_before += int((tau * hz > 0).sum())
    assert n_before > 100 and n_rejected > 100
    print('%s: %d records compared, %d births before a series, %d lives rejected' % (name, total, n_before, n_rejected))


# ---- 2. off == today; at the peak == no series ---------------------------------------------------------------------
@pytest.mark.parametrize("name,model,rig,traj", CASES, ids=CASE_IDS)
def test_no_series_and_a_series_at_its_peak_give_todays_bytes(sdb, name, model, rig, traj):
    frames = [0, 2]
    opt, sims, dgrid, cdf, kw, cam, box = cases.case_run(model, rig, traj, frames)
    hz = float(opt['cam_hz'])
    at_peak = R(0, [PEAK] * 4)
    assert at_peak.peak == PEAK and at_peak.dlam().tobytes() == np.zeros(4).tobytes()
    above = R(0, [PEAK] * 4, peak=PEAK)
    gusts = particles.gust_series(3, HZ, 4.0, 2.0, seed=5)
    for air in (dict(wind=(0.0, 0.0)), dict(wind=(-7.5, 2.0), gusts=gusts)):
        for draws, jit in (('stream', 0.0), ('counter', 5.0)):
            a = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, **air, **kw)
            b = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, rate_series=None, **air, **kw)
            c = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, rate_series=at_peak, **air, **kw)
            d = particles.expected_records(sims, dgrid, cdf, sdb, draws=draws, jitter=jit, rate_series=above, **air, **kw)
            assert all(len(x) > 100 and x.tobytes() == y.tobytes() == z.tobytes() == w.tobytes() for x, y, z, w in zip(a, b, c, d))
        V = len(rig) if rig is not None else 1
        tab = np.ascontiguousarray(cdf[0])
        for i, s in enumerate(sims):
            a = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, i % V, box, **air)
            for series in (None, at_peak):
                b = _all_slots(model, cam, dgrid, tab, s, hz, rig, traj, i % V, box, rate_series=series, **air)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            if model == 'rig':
                n, k = int(s['n_particles']), int(s['frame'])
                seed = int(s['key0']) | (int(s['key1']) << 32)
                sa = particles.rig_state(cam, dgrid, tab, n, k, seed, hz, tuple(box), **air)
                sb = particles.rig_state(cam, dgrid, tab, n, k, seed, hz, tuple(box), rate_series=None, **air)
                sc = particles.rig_state(cam, dgrid, tab, n, k, seed, hz, tuple(box), rate_series=at_peak, **air)
                assert set(sa) == set(sb) and all(sa[key].tobytes() == sb[key].tobytes() == sc[key].tobytes() for key in sa)
                assert sc['alive'].all()
    opt2 = cases.options('kitti')
    if model == 'field':
        a = particles.generate(opt2, 25, 2, seed=3, model='field')
        for series in (None, at_peak):
            b = particles.generate(opt2, 25, 2, seed=3, model='field', rate_series=series)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            fa, fb = particles.field_frame(opt2, 25, 2, seed=3), particles.field_frame(opt2, 25, 2, seed=3, rate_series=series)
            assert fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes()
    else:
        a = particles.rig_frame(opt2, 25, 1, rig, 0, seed=3, trajectory=traj)
        for series in (None, at_peak):
            b = particles.rig_frame(opt2, 25, 1, rig, 0, seed=3, trajectory=traj, rate_series=series)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 3. the law ----------------------------------------------------------------------------------------------------
def test_a_thinned_field_has_the_law_of_the_field_at_the_lower_rate():
    """Slots and tables at 100 mm/hr, thinned by a series constant at 25 mm/hr: over cases.N_LAW independent frames (a seed each, as
    cases._sample takes them) the kept count is within four standard errors of expected_count(cam, 25), and diameter, depth and image
    position pass cases._same_law -- its bounds, unchanged -- against plain 25 mm/hr fields of other seeds."""
    opt = cases.options('kitti')
    cam = particles.FrameCamera(opt, 0)
    rs = R(0, [25.0] * (7 * cases.N_LAW + 5), peak=100.0)
    counts, D, depth, px, py = [], [], [], [], []
    for i in range(cases.N_LAW):                                  # cases._sample('field', 9000) at the peak, under the series
        rec, _ = particles.field_frame(opt, 100, 7 * i + 3, seed=9000 + i, rate_series=rs)
        counts.append(len(rec))
        D.append(rec['wd1'] * 1e3)
        depth.append(-rec['wp1'][:, 2])
        px.append(rec['ip1'][:, 0])
        py.append(rec['ip1'][:, 1])
    thin = dict(cam=cam, counts=np.array(counts), D=np.concatenate(D), depth=np.concatenate(depth), px=np.concatenate(px), py=np.concatenate(py))
    plain_a, plain_b = cases._sample('field', 3000), cases._sample('field', 5000)
    control = cases._same_law(plain_a, plain_b)
    assert all(v < 1 for v in control.values()), control
    mean = particles.expected_count(cam, 25)[0]
    print('kept count: mean %.1f against expected_count %.1f, four standard errors %.1f' % (thin['counts'].mean(), mean, 4 * np.sqrt(mean / cases.N_LAW)))
    assert abs(thin['counts'].mean() - mean) < 4 * np.sqrt(mean / cases.N_LAW)
    got, got_b = cases._same_law(thin, plain_a), cases._same_law(thin, plain_b)
    print('statistic / threshold -- field vs field: %s\n  thinned vs field: %s\n  thinned vs field (other seeds): %s' % (control, got, got_b))
    assert all(v < 1 for v in got.values()), got
    assert all(v < 1 for v in got_b.values()), got_b
    # the test can tell: the peak's field itself has four times the count and larger drops
    peak = dict(thin)
    rec = [particles.field_frame(opt, 100, 7 * i + 3, seed=9000 + i)[0] for i in range(cases.N_LAW)]
    peak['counts'] = np.array([len(r) for r in rec])
    peak['D'] = np.concatenate([r['wd1'] * 1e3 for r in rec])
    bad = cases._same_law(peak, plain_a)
    assert bad['count'] > 1 and bad['D'] > 1, bad


# ---- 4. coherence --------------------------------------------------------------------------------------------------
N_RAMP = 40
FAST_HZ = 100.0     # KITTI's boxes are low (z_max = D f / pixel: 0.4 to 4.3 m): at its own 10 frames/s a fall lasts one to three
                    # frames and few lives are seen twice.  Items 4 and 5 film the same field at 100 frames/s: 10 to 30 frames per fall.


def _ramp():
    return R(0, np.linspace(25.0, 5.0, N_RAMP + 1))


def test_a_ramp_keeps_or_drops_a_life_for_good_and_kept_tracks_move_by_the_velocity():
    """25 -> 5 mm/hr over 40 frames.  The decision belongs to the (slot, life): its birth time m - tau cam_hz is the same number in
    every frame of the life up to the rounding of tau, so a life kept in frames k and k + 1 without the series is kept in both or
    in neither with it.  The tracks that stay move by cases._track_bounds' displacement: the series touches no position.  (FAST_HZ.)"""
    rs = _ramp()
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([50.0])}, cam_hz=FAST_HZ)
    cam = particles.FrameCamera(opt, 0)
    _, dgrid, cdf, _ = particles.expected_count(cam, 25)
    dt = 1.0 / cam.hz
    plain = [particles.field_frame(opt, 25, k, seed=11) for k in range(N_RAMP)]
    thin = [particles.field_frame(opt, 25, k, seed=11, rate_series=rs) for k in range(N_RAMP)]
    both = neither = tracked = 0
    for k in range(N_RAMP - 1):
        (pa, la), (pb, lb) = plain[k], plain[k + 1]
        (ta, tla), (tb, tlb) = thin[k], thin[k + 1]
        assert np.isin(ta['pid'], pa['pid']).all() and np.isin(tb['pid'], pb['pid']).all()
        _, ia, ib = np.intersect1d(pa['pid'], pb['pid'], return_indices=True)
        same = la[ia] == lb[ib]
        pid = pa['pid'][ia][same]                              # (slot, life) kept in both frames without the series
        in_a, in_b = np.isin(pid, ta['pid']), np.isin(pid, tb['pid'])
        assert np.array_equal(in_a, in_b), (k, int((in_a != in_b).sum()))
        both += int(in_a.sum())
        neither += int((~in_a).sum())
        # the kept records are the plain ones, byte for byte
        assert ta.tobytes() == pa[np.isin(pa['pid'], ta['pid'])].tobytes()
        _, ja, jb = np.intersect1d(ta['pid'], tb['pid'], return_indices=True)
        ok = (tla[ja] == tlb[jb]) & (ta['wp1'][ja, 2] < -0.05) & (tb['wp1'][jb, 2] < -0.05)
        ja, jb = ja[ok], jb[ok]
        if len(ja) == 0:
            continue
        vel, box = particles.field_kinematics(cam, dgrid, cdf, ta['pid'][ja], tla[ja], 11)
        r = (tb['wp1'][jb] - ta['wp1'][ja]) - vel * dt
        r[:, 0] -= box[:, 0] * np.rint(r[:, 0] / box[:, 0])
        r[:, 2] -= box[:, 2] * np.rint(r[:, 2] / box[:, 2])
        bound = cases._track_bounds(vel, box, tla[ja], dt)
        assert np.all(np.abs(r) <= bound), (k, (np.abs(r) / bound).max(axis=0))
        tracked += len(ja)
    print('ramp: %d (slot, life) pairs kept in both frames, %d in neither, %d tracks checked' % (both, neither, tracked))
    assert both > 1000 and neither > 1000 and tracked > 1000, (both, neither, tracked)


def _expected_kept(cam, rs, k, n_age=256):
    """The statement's own expected count at time index k: expected_count at the peak times the mean keep probability, the
    diameter drawn from the peak's sampling table and the age uniform in [0, 1) of the fall period T(D) = box height / v(D) -- the
    rate a frame shows is the rate at its drops' births.  Midpoint quadrature in both."""
    total, dgrid, cdf, z_max = particles.expected_count(cam, rs.peak)
    L = rs.dlam()
    hy = ((0.5 + 0.05) * float(cam.H)) / cam.fpx
    Dm = 0.5 * (dgrid[1:] + dgrid[:-1])
    w = np.diff(cdf)
    T = 2.0 * (hy * np.minimum(Dm * 1e-3 * cam.fpx, 15.0)) / particles.terminal_velocity(Dm)
    age = (np.arange(n_age) + 0.5) / n_age
    sb = np.maximum((k - rs.frame0) - age[None, :] * T[:, None] * cam.hz, 0.0)
    i = np.floor(sb).astype(np.int64)
    Lb = L[i] + (sb - i) * (L[i + 1] - L[i])
    return total * float((w * np.exp(-Lb * Dm[:, None]).mean(axis=1)).sum())


def test_the_count_follows_the_rate():
    """The ramp's first and last ten frames, every frame under a seed of its own (independent frames: a Poisson count each), against
    expected_count at their rates.  The rate a frame shows is the rate at its drops' BIRTH times (not promised: the lag
    of up to one fall period), so the expectation is taken where the statement takes it -- _expected_kept, expected_count at the
    peak times the mean keep probability over diameter and age -- and lies between expected_count at the frame's own rate and at
    the peak, which the test also checks.  Bound: four standard errors of a mean of ten Poisson counts, sqrt(mean / 10) -- against
    the statement's expectation and against expected_count at the frames' own rates alike (at KITTI's 10 frames/s a fall lasts one
    to three frames, and the lag moves the expectation by 6 to 8 drops of 220 to 560)."""
    rs = _ramp()
    opt = cases.options('kitti')
    cam = particles.FrameCamera(opt, 0)
    means, wants = [], []
    for frames in (range(0, 10), range(N_RAMP - 10, N_RAMP)):
        got = np.array([len(particles.field_frame(opt, 25, k, seed=700 + k, rate_series=rs)[0]) for k in frames])
        want = np.array([_expected_kept(cam, rs, k) for k in frames])
        now = np.array([particles.expected_count(cam, rs.rate_at(k))[0] for k in frames])
        print('frames %d .. %d: mean count %.1f, expected %.1f (at the frames\' own rates %.1f), four standard errors %.1f'
              % (frames[0], frames[-1], got.mean(), want.mean(), now.mean(), 4 * np.sqrt(want.mean() / 10)))
        assert np.all(np.diff(want) <= 0) and np.all(want >= now * (1 - 1e-9))                      # non-increasing; never below the frame's own rate
        assert np.all(want <= particles.expected_count(cam, 25)[0] * (1 + 1e-9))
        assert abs(got.mean() - want.mean()) < 4 * np.sqrt(want.mean() / 10)
        assert abs(got.mean() - now.mean()) < 4 * np.sqrt(now.mean() / 10)       # and of expected_count at the frames' own rates: the lag is inside
        means.append(got.mean())
        wants.append(want.mean())
    assert means[0] > means[1] and wants[0] > wants[1]
    # at a constant rate the quadrature is expected_count itself
    flat = R(0, [10.0] * 4, peak=25.0)
    assert abs(_expected_kept(cam, flat, 2) / particles.expected_count(cam, 10)[0] - 1) < 2e-3


# ---- 5. a dry spell ------------------------------------------------------------------------------------------------
def test_a_dry_spell_empties_the_field_after_the_longest_fall_period():
    """The rate is 25 up to time index 2 and 0 from index 3 on.  A life born at or after index 3 is never admitted (L = 100), so a
    frame k > 3 holds only drops at least (k - 3) / cam_hz old, and none once that exceeds the longest fall period of the settings
    -- computed here from field_kinematics' boxes and velocities.  (FAST_HZ.)"""
    opt = cases.options('kitti', cam_hz=FAST_HZ)
    cam = particles.FrameCamera(opt, 0)
    _, dgrid, cdf, _ = particles.expected_count(cam, 25)
    n_slots = int(particles.field_slot_counts(opt, 25, 1, 11)[0])
    vel, box = particles.field_kinematics(cam, dgrid, cdf, np.arange(n_slots), np.zeros(n_slots), 11)
    T_max = float((box[:, 1] / np.abs(vel[:, 1])).max())
    k_dry = 3 + int(np.ceil(T_max * FAST_HZ)) + 1
    rs = R(0, [25.0, 25.0, 25.0] + [0.0] * (k_dry + 2))
    key = particles._key(11)
    hy = ((0.5 + 0.05) * float(cam.H)) / cam.fpx
    assert len(particles.field_frame(opt, 25, 2, seed=11, rate_series=rs)[0]) == len(particles.field_frame(opt, 25, 2, seed=11)[0])
    left = []
    for k in (4, 5, 6):
        rec, life = particles.field_frame(opt, 25, k, seed=11, rate_series=rs)
        left.append(len(rec))
        j = rec['pid'].astype(np.uint64)
        D, phase, _, z_max = particles._slot_draw(cam, dgrid, cdf, j, key, 1.0, 15.0)
        tau = particles._slot_fall(cam, FAST_HZ, k, j, key, D, 2.0 * (hy * z_max), phase, 1.0)[3]
        assert len(rec) > 100 and np.all(tau * FAST_HZ >= (k - 3) - 1e-9), (k, len(rec))
    assert left[0] > left[1] > left[2]
    for k in (k_dry, k_dry + 1):
        assert len(particles.field_frame(opt, 25, k, seed=11, rate_series=rs)[0]) == 0
        assert len(particles.field_frame(opt, 25, k, seed=11)[0]) > 100
    print('longest fall period %.2f s: frames 4, 5, 6 keep %s records, frame %d none' % (T_max, left, k_dry))


# ---- 6. the rig ----------------------------------------------------------------------------------------------------
def test_both_stereo_views_keep_the_same_lives():
    rs = cases.rate_cases()[1][0]
    rig = cases.KITTI_STEREO
    opt = cases.options('kitti')
    seen = rejected = 0
    for k in (0, 5):
        a = [particles.rig_frame(opt, 25, k, rig, v, seed=3) for v in (0, 1)]
        b = [particles.rig_frame(opt, 25, k, rig, v, seed=3, rate_series=rs) for v in (0, 1)]
        common = np.intersect1d(a[0][0]['pid'], a[1][0]['pid'])
        k0, k1 = np.isin(common, b[0][0]['pid']), np.isin(common, b[1][0]['pid'])
        assert np.array_equal(k0, k1)
        for v in (0, 1):                                        # the kept records are the plain ones, with their lives
            sel = np.isin(a[v][0]['pid'], b[v][0]['pid'])
            assert np.isin(b[v][0]['pid'], a[v][0]['pid']).all()
            assert a[v][0][sel].tobytes() == b[v][0].tobytes() and a[v][1][sel].tobytes() == b[v][1].tobytes()
        seen += int(k0.sum())
        rejected += int((~k0).sum())
    assert seen > 100 and rejected > 100, (seen, rejected)


# ---- 7. shower_series, refusals, the driver and the augmenter -----------------------------------------------------
def test_shower_series():
    a = particles.shower_series(80, HZ, 25.0, 2.0, 4.0)
    i = np.arange(81)
    want = 2.0 + (25.0 - 2.0) * (1.0 - np.cos(2.0 * np.pi * (i / HZ) / 4.0 + 0.0)) / 2.0
    assert a.frame0 == 0 and a.n == 80 and a.peak == 25.0 and a.rate.shape == (81,)
    assert np.array_equal(a.rate, np.minimum(want, 25.0)) and a.rate[0] == 2.0 and abs(a.rate[20] - 25.0) < 1e-12 and abs(a.rate[40] - 2.0) < 1e-12
    assert a.rate.max() <= 25.0 and a.rate.min() >= 2.0
    b = particles.shower_series(8, HZ, 25.0, 0.0, 4.0, frame0=BIG0, phase=np.pi)
    assert b.frame0 == BIG0 and b.rate[0] == 25.0 and b.covers([BIG0, BIG0 + 7]).all() and not b.covers([BIG0 - 1, BIG0 + 8]).any()
    assert b.rate_at(BIG0) == 25.0
    # the table: 0 at the peak, the cap at rate 0, Lambda's excess in between
    L = particles.shower_series(40, HZ, 25.0, 0.0, 4.0).dlam()
    assert L[20] < 1e-12 and L[0] == particles.RATE_DLAM_MAX == 100.0 and np.all(L >= 0) and np.all(L <= 100.0)
    assert L[10] == particles.mp_lambda(particles.shower_series(40, HZ, 25.0, 0.0, 4.0).rate[10]) - particles.mp_lambda(25.0)
    assert R(0, [1e-30, 25.0]).dlam()[0] == 100.0              # a rate so small that Lambda's excess is beyond the cap
    # the two constants of the statement
    assert float(particles.det_exp(-(0.0 * 6.0))) == 1.0 and float(particles.det_exp(-(100.0 * 0.5))) < 2.0 ** -33
    for bad in (dict(n=0), dict(n=2 ** 20 + 1), dict(cam_hz=0.0), dict(peak=0.0), dict(low=-1.0), dict(low=26.0), dict(period_s=0.0),
                dict(phase=float('nan')), dict(peak=float('inf'))):
        kw = dict(n=4, cam_hz=HZ, peak=25.0, low=2.0, period_s=4.0)
        kw.update(bad)
        with pytest.raises(ValueError, match='shower_series'):
            particles.shower_series(**kw)


def test_refusals(sdb):
    ok = [25.0, 10.0, 0.0]
    assert particles._check_rate_series(None, 'iid') is None
    assert particles._check_rate_series(R(0, ok)).n == 2
    particles._check_rate_series(R(2 ** 32 - 2, ok))                                   # frame0 + n = 2^32 is allowed
    particles._check_rate_series(R(0, ok, peak=25.0))                                  # a peak equal to max(rate) is allowed
    bad = [R(2 ** 32 - 1, ok), R(-1, ok), R(0, ok[:1]), R(0, np.zeros((3, 2))), R(0, [25.0, np.nan]), R(0, [25.0, np.inf]),
           R(0, [25.0, -1.0]), R(0, ok, peak=24.0), R(0, [0.0, 0.0]), R(0, ok, peak=float('inf')), (0, ok), 'showers']
    for r in bad:
        with pytest.raises(ValueError, match='rate'):
            particles._check_rate_series(r)
    with pytest.raises(ValueError, match='2\\^20'):
        particles._check_rate_series(R(0, np.ones(2 ** 20 + 2)))
    with pytest.raises(ValueError, match='no time'):
        particles._check_rate_series(R(0, ok), 'iid')
    # the generator's: the i.i.d. model, a frame outside the series, run_pos
    opt = cases.options('kitti')
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1)
    with pytest.raises(ValueError, match='no time'):
        particles.expected_records(sims, dgrid, cdf, sdb, rate_series=R(0, ok))
    with pytest.raises(ValueError, match='no time'):
        particles.generate(opt, 25, 1, rate_series=R(0, ok))
    opt, fs, dgrid, cdf, kw, cam, box = cases.case_run('field', None, None, [2])
    with pytest.raises(ValueError, match='outside the rate series'):
        particles.expected_records(fs, dgrid, cdf, sdb, rate_series=R(0, ok), **kw)
    with pytest.raises(ValueError, match='outside the rate series'):
        particles.expected_records(fs, dgrid, cdf, sdb, rate_series=R(3, ok), **kw)
    assert len(particles.expected_records(fs, dgrid, cdf, sdb, rate_series=R(1, ok), **kw)[0]) > 100
    with pytest.raises(ValueError, match='outside the rate series'):
        particles.field_frame(opt, 25, 2, rate_series=R(0, ok))
    with pytest.raises(ValueError, match='outside the rate series'):
        particles.generate(opt, 25, 3, model='field', rate_series=R(0, ok))
    with pytest.raises(ValueError, match='outside the rate series'):
        particles.rig_frame(opt, 25, 2, cases.MONO, 0, rate_series=R(0, ok))
    runp = fs.copy()
    runp['run_pos'] = 1
    with pytest.raises(ValueError, match='run_pos'):
        particles.expected_records(runp, dgrid, cdf, sdb, rate_series=R(1, ok), **kw)
    with pytest.raises(ValueError, match='no angular noise'):
        particles.expected_records(fs, dgrid, cdf, sdb, noise_std=2.0, noise_scale=1.0, rate_series=R(1, ok), **kw)


def test_the_driver_and_the_augmenter_carry_the_series(tmp_path):
    """--showers LOW,PERIOD_S[,PHASE]: parsed next to --gusts, needs the field or rig model, leaves --streak_lean alone;
    RainAugment.plan carries the series and every image's own fog constants, and refuses what the series does not cover."""
    main = importlib.import_module('rain-rendering_amd.main')
    add_attenuation = importlib.import_module('rain-rendering_amd.common.add_attenuation')
    common = ['--dataset', 'kitti', '-k', str(tmp_path), '-i', '25']
    field = ['--device_particles', '--particle_model', 'field']

    def parsed(extra):
        ns = main._wind_and_lean(main._parse(common + extra))
        return ns.showers, ns.lean
    assert parsed([]) == (None, False) and parsed(field) == (None, False)
    assert parsed(field + ['--showers', '2,4']) == ((2.0, 4.0, 0.0), False)
    assert parsed(field + ['--showers', '0,4,1.5', '--wind', '3,0']) == ((0.0, 4.0, 1.5), True)
    assert parsed(field + ['--showers', '25,0.5', '--gusts', '3']) == ((25.0, 0.5, 0.0), True)
    for bad in ([], ['--device_particles'], field + ['--showers=2'], field + ['--showers=-1,4'], field + ['--showers=26,4'],
                field + ['--showers=2,0'], field + ['--showers=2,4,1,1'], field + ['--showers=a,4'], field + ['--showers=2,4,nan'],
                field + ['--showers=inf,4']):
        with pytest.raises(SystemExit, match='--showers'):
            main._derive(main._parse(common + (bad if any(b.startswith('--showers') for b in bad) else bad + ['--showers', '2,4'])))
    augment = importlib.import_module('rain-rendering_amd.augment')
    root = str(tmp_path)
    h.synthetic.write_streak_db(os.path.join(root, 'rainstreakdb'))
    kw = dict(streaks_db=os.path.join(root, 'rainstreakdb'), sequence='data_object/training')
    rs = particles.shower_series(12, HZ, 25.0, 0.0, 1.2)
    aug = augment.RainAugment('kitti', particle_model='field', draws='counter', showers=rs, **kw)
    p = aug.plan(None, [6, 0, 11])
    assert p['showers'] is rs and p['lean'] is False and p['key'] == (25.0,)
    same = aug.plan(25, [6, 0, 11])
    assert same['sims'].tobytes() == p['sims'].tobytes() and same['fog'].tobytes() == p['fog'].tobytes()
    plain = augment.RainAugment('kitti', particle_model='field', draws='counter', **kw).plan(25, [6, 0, 11])
    assert plain['sims'].tobytes() == p['sims'].tobytes() and plain['cdf'].tobytes() == p['cdf'].tobytes()      # slots and tables: the peak's
    assert plain['drops_cap'] == p['drops_cap'] and plain.get('showers') is None
    for i, f in enumerate([6, 0, 11]):                         # image i's fog constants are FogRain(rate at frame_index[i])'s
        fog = add_attenuation.FogRain(rain_intensity=rs.rate_at(f), focal=aug.focal, f_number=aug.f_number, angle=90, exposure=aug.exposure,
                                      camera_gain=aug.camera_gain).constants()
        assert p['fog'][i].tobytes() == np.asarray(fog, np.float64).tobytes()
    assert p['fog'][0].tobytes() == plain['fog'][0].tobytes() and p['fog'][1, 0] == 0.0 and p['fog'][2, 0] < p['fog'][0, 0]
    recs = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws=p['draws'],
                                      rate_series=p['showers'])
    full = particles.expected_records(p['sims'], p['d_grid'], p['cdf'], aug.db, model='field', cam_hz=p['cam_hz'], draws=p['draws'])
    assert 100 < len(recs[0]) < len(full[0]) and len(recs[1]) < len(recs[0])
    with pytest.raises(ValueError, match='outside the rate series'):
        aug.plan(None, [4, 12])
    with pytest.raises(ValueError, match='intensity'):
        aug.plan(10, [4, 5])
    with pytest.raises(ValueError, match='intensity'):
        aug.plan([25, 10], [4, 5])
    aug.set_showers(None)
    assert aug.plan(25, [4, 12])['showers'] is None
    with pytest.raises(ValueError, match='intensity'):
        aug.plan(None, [4, 5])
    aug.set_showers(rs)
    assert aug.plan(None, [4])['showers'] is rs
    rig_aug = augment.RainAugment('kitti', particle_model='rig', rig=cases.KITTI_STEREO, showers=rs, **kw)
    pr = rig_aug.plan(None, [6, 0])
    assert pr['showers'] is rs and pr['fog'].shape == (4, 4) and pr['fog'][0].tobytes() == pr['fog'][1].tobytes() == p['fog'][0].tobytes()
    for bad in ('showers', (0, rs.rate), particles.RateSeries(0, [25.0, -1.0]), particles.RateSeries(0, [25.0, 5.0], peak=20.0)):
        with pytest.raises(ValueError, match='rate'):
            augment.RainAugment('kitti', particle_model='field', showers=bad, **kw)
    with pytest.raises(ValueError, match='no time'):
        augment.RainAugment('kitti', showers=rs, **kw)
