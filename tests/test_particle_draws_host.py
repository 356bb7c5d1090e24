"""CPU tier: counter-based per-drop draws (tools/particles.py counter_picks / expected_records(draws='counter'), rr_particles.h
texture_pick, rr_set_particle_draws) -- the texture pick from the drop's own Philox counter instead of numpy's stream.

  1. the g++ build of the RR_HD statement (tests/hostemu/particles_emu.cpp: the code the counter-mode kernels run) == numpy, bit
     for bit, for the i.i.d., field and rig models;
  2. coherence: a field slot keeps its pick from frame k to k + 1 inside one life, a rig slot in both stereo views of an instant;
     the stream mode's picks of the same pairs agree about one time in ten (the control);
  3. law: the ten picks are equally likely (chi-square, both modes through the same threshold);
  4. the counter mode changes tex_index only, and only its last decimal digit;
  5. every refusal of the Python layer and of the driver's argument handling."""
import importlib

import numpy as np
import pytest

import helpers as h
import particle_cases as cases
import particle_emu as pe

particles = importlib.import_module('rain-rendering_amd.tools.particles')

CHI2_9_999 = 27.88                                        # chi-square, 9 degrees of freedom: P(X > 27.88) = 0.001


@pytest.fixture(scope='module')
def emu(built):
    return pe.load()


# ---- 1. g++ == numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ['iid', 'field', 'rig'])
def test_gxx_build_equals_numpy(tmp_path, emu, model):
    sc = h.Scene(tmp_path, 64, 96, 10)                       # (only its streak database is used: the texture ratios)
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([30.0])})
    hz = float(opt['cam_hz'])
    rig = cases.KITTI_STEREO if model == 'rig' else None
    V = len(rig) if rig is not None else 1
    seed = 1234 + 2 ** 40
    sims, dgrid, cdf, kw = cases.run(model, opt, 25, [0, 1, 2 ** 31 + 5], seed, rig)
    want = particles.expected_records(sims, dgrid, cdf, sc.db, draws='counter', **kw)
    assert len(want) == 3 * V
    W, H = opt["cam_CCD_WH"]
    ratio_db = np.ascontiguousarray(np.asarray(sc.db.ratio, np.float64)[:4])
    tab = np.ascontiguousarray(cdf[0])
    cam = particles.FrameCamera(opt, 0)
    box = np.array(rig.box(cam), np.float64) if rig is not None else np.zeros(3)
    views = rig.as_records() if rig is not None else None
    total = 0
    for i, s in enumerate(sims):
        n = int(s['n_particles'])
        view = views[i % V:i % V + 1] if views is not None else None
        run = pe.run(model=model, sim=sims[i:i + 1], cam_hz=hz, view=view, box=box, dgrid=dgrid, cdf=tab, counter=True)
        # the pick of every particle / slot, kept or not
        _, _, life, pick = pe.all_slots(run)
        if model == 'iid':
            ref = particles.counter_picks(seed, np.arange(n), frame=int(s['frame']))
        elif model == 'field':
            _, g = particles.make_field_particles(cam, dgrid, tab, n, int(s['frame']), seed, hz, cull=False)
            assert np.array_equal(life, g)
            ref = particles.counter_picks(seed, np.arange(n), life=g)
        else:
            g = particles.rig_state(cam, dgrid, tab, n, int(s['frame']), seed, hz, box)['life']
            assert np.array_equal(life, g)
            ref = particles.counter_picks(seed, np.arange(n), life=g)
        assert np.array_equal(pick, ref) and 0 <= pick.min() and pick.max() <= 9 and len(set(pick.tolist())) == 10
        # the finished records
        out, _ = pe.records(run, H, W, ratio_db)
        k = len(out)
        assert k == len(want[i]) > 100, (i, k, len(want[i]))
        pe.assert_records_equal(out, want[i], 'counter', i)
        total += k
    print('%s: %d records compared' % (model, total))


def test_texture_pick_is_the_scaled_word():
    w = np.array([0, 1, 429496729, 429496730, 2 ** 31, 2 ** 32 - 1], np.uint64)
    assert particles.texture_pick(w).tolist() == [0, 0, 0, 1, 5, 9] == [int(x) * 10 >> 32 for x in w]


# ---- 2. coherence --------------------------------------------------------------------------------------------------
N_CLIP = 40


@pytest.fixture(scope='module')
def clips(tmp_path_factory):
    """Per mode the picks of (a) a 40-frame field clip and (b) 40 stereo instants: lists of {slot: (life, pick)} per frame."""
    sc = h.Scene(tmp_path_factory.mktemp('draws'), 64, 96, 10)
    opt = cases.options('kitti', sim_steps={"cam_motion": np.array([30.0])})
    frames = 50 + np.arange(N_CLIP)
    out = {}
    for model, rig in (('field', None), ('rig', cases.KITTI_STEREO)):
        sims, dgrid, cdf, kw = cases.run(model, opt, 25, frames, 77, rig)
        V = 2 if rig is not None else 1
        ids = [cases.kept(s, dgrid, cdf, sc.db, model, opt['cam_hz'], rig, i % V) for i, s in enumerate(sims)]
        for draws in ('stream', 'counter'):
            recs = particles.expected_records(sims, dgrid, cdf, sc.db, draws=draws, **kw)
            per = []
            for (pid, life), r in zip(ids, recs):
                assert len(pid) == len(r)
                per.append({int(j): (float(g), int(t) % 10, int(t) // 10) for j, g, t in zip(pid, life, r['tex_index'])})
            out[model, draws] = per
    return out


def _pairs(per, step, stride):
    """(same life, pick a, pick b, bucket a, bucket b) of every slot kept by frames i and i + step, i = 0, stride, 2 stride ..."""
    rows = []
    for i in range(0, len(per) - step, stride):
        a, b = per[i], per[i + step]
        for j in sorted(set(a) & set(b)):
            rows.append((a[j][0] == b[j][0], a[j][1], b[j][1], a[j][2], b[j][2]))
    return np.array(rows, np.int64)


@pytest.mark.parametrize("model,step,stride", [('field', 1, 1), ('rig', 1, 2)], ids=['field-next-frame', 'rig-other-view'])
def test_a_drop_keeps_its_pick(clips, model, step, stride):
    """Field: a slot kept in frames k and k + 1 in one life.  Rig: a slot kept by both stereo views of one instant (records 2 i
    and 2 i + 1; one instant is one life).  Counter draws: the same pick, always.  Stream draws, the same pairs: the picks are
    independent, agreeing one time in ten -- at most half is asked."""
    ctr, strm = _pairs(clips[model, 'counter'], step, stride), _pairs(clips[model, 'stream'], step, stride)
    assert len(ctr) == len(strm) and np.array_equal(ctr[:, 0], strm[:, 0])          # the same pairs
    same = ctr[:, 0] == 1
    n = int(same.sum())
    print('%s: %d pairs in one life, %d across lives' % (model, n, int((~same).sum())))
    assert n >= 200
    assert np.array_equal(ctr[same, 1], ctr[same, 2])
    agree = float(np.mean(strm[same, 1] == strm[same, 2]))
    print('%s: stream picks agree in %.3f of the pairs' % (model, agree))
    assert agree <= 0.5
    if model == 'rig':
        assert same.all()                                    # (one instant is one life)


def test_a_new_life_is_a_new_drop():
    """Across lives nothing is promised -- and nothing is shared: over many slots the picks of two lives agree like chance."""
    seed, n = 5, 20000
    j = np.arange(n)
    a = particles.counter_picks(seed, j, life=np.full(n, 3.0))
    b = particles.counter_picks(seed, j, life=np.full(n, 4.0))
    c = particles.counter_picks(seed, j, life=np.full(n, 3.0 + 2.0 ** 32))       # g_hi enters the counter
    assert 0.07 < np.mean(a == b) < 0.13 and 0.07 < np.mean(a == c) < 0.13
    assert np.array_equal(a, particles.counter_picks(seed, j, life=np.full(n, 3.0)))
    assert not np.array_equal(a, particles.counter_picks(seed + 1, j, life=np.full(n, 3.0)))


# ---- 3. law --------------------------------------------------------------------------------------------------------
def _chi2(picks):
    cnt = np.bincount(picks, minlength=10).astype(np.float64)
    e = cnt.sum() / 10.0
    return float(((cnt - e) ** 2 / e).sum()), int(cnt.sum())


@pytest.mark.parametrize("model", ['iid', 'field'])
def test_the_ten_picks_are_equally_likely(tmp_path, model):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('nuscenes')
    # chi-square asks for independent samples: under the field model a drop shows in every frame of its life with the one pick
    # (that is the point of the mode), so the field's frames are taken 1000 apart -- no life lasts that long (the tallest box
    # is crossed in about a second), every record is then a drop of its own
    frames = [3, 4, 5, 6, 7] if model == 'iid' else [3, 1003, 2003, 3003, 4003]
    sims, dgrid, cdf, kw = cases.run(model, opt, 100, frames, 2024)
    for draws in ('counter', 'stream'):                      # (the stream mode goes through the same threshold: the control)
        recs = particles.expected_records(sims, dgrid, cdf, sc.db, dataset='nuscenes', draws=draws, **kw)
        x2, n = _chi2(np.concatenate([r['tex_index'] % 10 for r in recs]))
        print('%s %s: chi2(9) = %.2f over %d drops' % (model, draws, x2, n))
        assert n >= 20000
        assert x2 < CHI2_9_999, (draws, x2)


# ---- 4. nothing else moves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ['iid', 'field', 'rig'])
def test_only_the_last_digit_of_tex_index_differs(tmp_path, model):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    rig = cases.KITTI_STEREO if model == 'rig' else None
    sims, dgrid, cdf, kw = cases.run(model, opt, 100, [7, 8], 11, rig)
    a = particles.expected_records(sims, dgrid, cdf, sc.db, draws='stream', **kw)
    b = particles.expected_records(sims, dgrid, cdf, sc.db, draws='counter', **kw)
    other = sims.copy()
    other['draw_seed'] += 1000                                # draw_seed is ignored
    c = particles.expected_records(other, dgrid, cdf, sc.db, draws='counter', **kw)
    for x, y, z in zip(a, b, c):
        assert len(x) == len(y) > 100
        for name in h.hb.DROP_DTYPE.names:
            if name != 'tex_index':
                assert x[name].tobytes() == y[name].tobytes(), name
        assert np.array_equal(x['tex_index'] // 10, y['tex_index'] // 10) and not np.array_equal(x['tex_index'], y['tex_index'])
        assert y.tobytes() == z.tobytes()
    assert particles.expected_records(sims, dgrid, cdf, sc.db, **kw)[0].tobytes() == a[0].tobytes()       # the default is the stream


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    sc = h.Scene(tmp_path, 64, 96, 10)
    opt = cases.options('kitti')
    sims, dgrid, cdf = particles.sim_frames(opt, 25, 1)
    with pytest.raises(ValueError, match='particle draws'):
        particles.expected_records(sims, dgrid, cdf, sc.db, draws='philox')
    with pytest.raises(ValueError, match='angular noise'):
        particles.expected_records(sims, dgrid, cdf, sc.db, draws='counter', noise_std=2.0, noise_scale=1.0, run=([0], [0]))
    bad = sims.copy()
    bad['run_pos'] = 1
    with pytest.raises(ValueError, match='run_pos'):
        particles.expected_records(bad, dgrid, cdf, sc.db, draws='counter')
    # the driver's argument handling (before it looks at any path)
    main = importlib.import_module('rain-rendering_amd.main')
    common = ['--dataset', 'kitti', '-k', str(tmp_path), '-i', '25']
    with pytest.raises(SystemExit, match='needs --device_particles'):
        main._derive(main._parse(common + ['--particle_draws', 'counter']))
    with pytest.raises(SystemExit, match='--noise_std cannot be combined with --particle_draws counter'):
        main._derive(main._parse(common + ['--particle_draws', 'counter', '--device_particles', '--noise_std', '2']))
    with pytest.raises(SystemExit):                           # argparse: not one of the choices
        main._parse(common + ['--particle_draws', 'mt19937'])
    assert main._parse(common).particle_draws == 'stream'


def test_rain_augment_validates_draws():
    augment = importlib.import_module('rain-rendering_amd.augment')
    with pytest.raises(ValueError, match='draws'):
        augment.RainAugment('kitti', streaks_db='/nonexistent', draws='philox')
