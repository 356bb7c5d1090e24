"""GPU tier: the software pipeline of k_blur_small past its first iteration.  One call of 256 small frames (the per-frame grid is
then 64 workgroups) that rotate the three drop tables of tests/blur_small_pipeline.py: waves run 0, 1, 2, 3 and 4 iterations,
waves of one workgroup leave in different iterations, and every branch of the row and the column pass is taken by a drop that
was prefetched while another drop, of another radius and another branch, was being filtered.  Every frame must equal the g++
build of the kernel arithmetic for its table (pinned to the oracle by tests/test_blur_small_pipeline_host.py): statuses and
both masks bit for bit, the image within 1 LSB; a failure names the drops under the differing pixels with their wave and
iteration."""
import numpy as np
import pytest

import blur_routes as br
import blur_small_pipeline as sp
import helpers as h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def case(built, tmp_path_factory):
    sc = h.Scene(tmp_path_factory.mktemp('small_pipeline'), sp.H, sp.W, 0, frames=sp.frames())
    inputs = [sc.frame_inputs(t) for t in range(3)]
    drops = [sc.product_drops(t) for t in range(3)]
    assert [len(d) for d in drops] == list(sp.N_TABLE)
    recs = [br.classify_drops(sc, d) for d in drops]
    refs = [h.emu_render(sc, inputs[t][0], inputs[t][0], inputs[t][1], drops[t]) for t in range(3)]
    frames = [dict(bg=inputs[t][0], rainy_bg=inputs[t][0], env_xyY=inputs[t][1], omega=sc.omega, drops=drops[t]) for t in range(3)]
    rh = h.hb.RainHip(0)
    try:
        rh.set_streak_db(sc.db.streaks_light)
        rh.set_camera(sc.cam)
        outs = rh.render_frames([frames[f % 3] for f in range(sp.N_FRAMES)])
        counts = [rh.batch_counts(f) for f in range(3)]
    finally:
        rh.close()
    return recs, refs, outs, counts


def test_census_holds_for_the_call(case):
    """The census is a condition of the comparison: no class empty, and the device's small lists as long as the census' ones."""
    recs, _, outs, counts = case
    found = sp.census(recs, n_frames=len(outs))
    assert not [k for k in sp.REQUIRED if not found[k]] and not found['neighbours_same_r1'], {k: len(v) for k, v in found.items()}
    assert len(outs) == sp.N_FRAMES and sp.grid_x(max(sp.N_TABLE), len(outs)) == 64
    for t in range(3):
        assert counts[t][2:5] == br.expected_counts(recs[t])[:3] == [0, 0, sp.N_TABLE[t]], (t, counts[t])


def test_every_frame_matches_its_table(case):
    recs, refs, outs, _ = case
    fails = {}                          # table: [differing pixels of its first failing frame, failing frames, message]
    for f, out in enumerate(outs):
        t = f % 3
        try:
            br.check(out, refs[t], recs[t], 'frame %d (table %s) vs hostemu' % (f, sp.TABLE_NAMES[t]))
        except AssertionError as e:
            if t in fails:
                fails[t][1] += 1
                continue
            diff = (out['mask'] != refs[t]['mask']) | (out['mask_i32'] != refs[t]['mask_i32']) | \
                   (np.abs(out['image_u8'].astype(int) - refs[t]['image_u8'].astype(int)) > 1).any(axis=2)
            fails[t] = [int(diff.sum()), 1, '%s\n  %s' % (e, '\n  '.join(sp.drops_explaining(recs[t], diff, max(sp.N_TABLE), len(outs))))]
    # the table with the fewest differing pixels first: its drops overlap least, so it names the culprit most sharply
    assert not fails, '\n'.join('%s\n  (%d frames of table %s differ)' % (m, n, sp.TABLE_NAMES[t])
                                for t, (_, n, m) in sorted(fails.items(), key=lambda kv: kv[1][0]))
    assert all(out['mask'].max() > 0 for out in outs)
