"""CPU tier of the PNG coder's catalogue (tests/pngz_cases.py): the catalogue and the reference on trial.

Every case is built, its scanlines formed the way k_png_image / k_png_mask form them, coded by the host build of rr_deflate.h
(emu_pngz) and held to zlib -- the GPU tier then holds the device to the emulation byte for byte, which is only worth something if
the emulation is right on these very inputs.  The trace (emu_pngz_trace) shows that each case lands where it aims: a catalogue
that misses its edges would pass on the device for the wrong reason."""
import zlib

import numpy as np
import pytest

import helpers as h
import pngz_cases as pc


def held_to_zlib(rows, total, dst):
    """What tests/test_deflate_hostemu.py asserts of a coded file: zlib inflates the stream to every byte (and checks its Adler-32)."""
    n = rows.size
    if total == 0:
        assert np.array_equal(dst, rows)                       # did not fit: the scanlines stay, first byte a filter type
        return
    assert dst[:4].tobytes() == pc.MAGIC and int(dst[4:8].view(np.uint32)[0]) == total and not dst[8:16].any()
    assert pc.HEADER + total <= n
    assert zlib.decompress(dst[16:16 + total].tobytes()) == rows.tobytes()
    assert np.array_equal(dst[16 + total:], rows[16 + total:])  # behind the stream: what was there


def test_byte_centres_survive_the_frame_pipeline_s_truncation():
    """rainy_bg = (k + 0.5) / 255 comes back as the byte k from trunc(v * 255), as a float64 and rounded to float32."""
    k = np.arange(256)
    v64 = (k + 0.5) / 255.0
    assert np.array_equal((v64 * 255.0).astype(np.int64), k)
    v32 = v64.astype(np.float32)
    assert np.array_equal((v32.astype(np.float64) * 255.0).astype(np.int64), k)
    assert np.array_equal((v32 * np.float32(255.0)).astype(np.int64), k)
    # the 16-bit composite code in between (k_composite32: rint(v * 65534) / 65534) moves a centre by less than half a byte
    code = np.rint(v32.astype(np.float64) * 65534.0) / 65534.0
    assert np.array_equal((code * 255.0).astype(np.int64), k)


def test_a_frame_without_drops_is_its_background_truncated(tmp_path):
    """The route of the catalogue on the host build of the frame arithmetic: image_u8 of a drop-less frame is the case's image."""
    case = pc.by_name('ladder-13x16')
    F, img, rows = pc.built(case)
    sc = h.Scene(tmp_path, case.H, case.W, 0)
    _, env = sc.frame_inputs(0)
    bg = pc.rainy_bg_of(img)
    out = h.emu_render(sc, bg, bg, env, np.zeros(0, h.hb.DROP_DTYPE))
    assert np.array_equal(out['image_u8'], img) and not out['mask'].any()


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_every_case_codes_to_what_zlib_inflates(case):
    F, img, rows = pc.built(case)
    assert rows.size == case.H * (1 + 4 * case.W)
    assert np.array_equal(pc.scanlines_rgb(img), rows), "numpy's Sub filter of the case's image is not the intended bytes"
    total, dst, tr = pc.emu_pngz(rows, trace=True)
    held_to_zlib(rows, total, dst)
    total2, dst2 = pc.emu_pngz(rows)
    assert total2 == total and np.array_equal(dst2, dst)      # the trace changes nothing
    assert int(tr['len'].sum()) == rows.size
    if total:
        assert total == 2 + int(tr['bytes'].sum()) + 4
    # the mask file of a frame without drops: index 0 of the colour map everywhere
    mrows = pc.scanlines_rgba(pc.mask_rgba(np.zeros((case.H, case.W)), pc.random_lut()))
    held_to_zlib(mrows, *pc.emu_pngz(mrows))


def test_small_files_stay_scanlines_up_to_a_threshold_the_emulation_finds():
    k_kept, k_coded, kept = pc.threshold_pair()
    assert 0 < k_kept and k_coded < len(pc.LADDER) - 1         # the pair lies inside the ladder: both sides are populated
    assert all(kept[:k_coded]) and not any(kept[k_coded:]), kept
    assert pc.LADDER[0] == (1, 1)
    for hw, kp in zip(pc.LADDER, kept):
        rows = pc.built(pc.by_name('ladder-%dx%d' % hw))[2]
        total, dst = pc.emu_pngz(rows)
        assert (dst[0] == 1 and np.array_equal(dst, rows)) if kp else dst[:4].tobytes() == pc.MAGIC


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.lands], ids=lambda c: c.name)
def test_edge_cases_land_on_their_edges(case):
    rows = pc.built(case)[2]
    total, dst, tr = pc.emu_pngz(rows, trace=True)
    assert total > 0
    n = rows.size
    assert len(tr) == (n + pc.BLOCK - 1) // pc.BLOCK
    for b, (stored, length) in case.lands['blocks'].items():
        assert (int(tr[b]['stored']), int(tr[b]['len'])) == (stored, length), (case.name, b)
        if stored:
            assert int(tr[b]['bytes']) == length + 5
    last = tr[-1]
    assert int((last['chunks'] == 0).sum()) == case.lands['idle'], (case.name, last['chunks'])
    assert int(last['chunks'].sum()) == (int(last['len']) + pc.CHUNK - 1) // pc.CHUNK


def test_tails_of_one_two_three_and_sixty_three_bytes_and_the_eighth_s_edges():
    """The last chunk of the file holds 1, 2, 3 and 63 bytes (nv < 64; with the flat content its equal bytes fall under the
    `L < 4` rule or not), and a last block ends on, one short of and one past a wave's eighth."""
    tails = sorted({(c.H * (1 + 4 * c.W)) % pc.CHUNK for c in pc.CASES if c.lands})
    assert {1, 2, 3, 63} <= set(tails), tails
    rests = {(c.H * (1 + 4 * c.W)) % pc.BLOCK for c in pc.CASES if c.lands}
    assert {pc.EIGHTH - 1, pc.EIGHTH, pc.EIGHTH + 1} <= rests
    for hw, tail in (((74, 27), 2), ((47, 43), 3), ((43, 47), 63)):
        rows = pc.built(pc.by_name('edge-%dx%d-flat' % hw))[2]
        assert not rows[-tail - 1:].any()                       # the tail continues a sequence of zeros from the chunk before it
        tr = pc.emu_pngz(rows, trace=True)[2]
        assert tr[-1]['seqs'][tail] >= 1                        # ... which the chunk's end cut to `tail` bytes
        if tail >= 4:
            assert tr[-1]['runs'][1, tail - 1] >= 1             # 63 bytes: one literal and a run of 62


def test_runs_of_every_length_begin_at_every_lane_and_are_cut_by_every_edge():
    runs = np.zeros((64, 64), np.int64)
    seqs = np.zeros(65, np.int64)
    cuts = np.zeros(3, np.int64)
    for c in pc.RUN_CASES:
        tr = pc.emu_pngz(pc.built(c)[2], trace=True)[2]
        coded = tr[tr['stored'] == 0]
        runs += coded['runs'].sum(axis=0)
        seqs += coded['seqs'].sum(axis=0)
        cuts += [coded['cut_chunk'].sum(), coded['cut_eighth'].sum(), coded['cut_block'].sum()]
    assert not runs[:, :3].any() and not runs[0].any()         # a run is 3..63 bytes behind its literal: never at lane 0
    assert (runs.sum(axis=0)[3:64] > 0).all(), np.flatnonzero(runs.sum(axis=0)[3:64] == 0) + 3
    assert (runs.sum(axis=1)[1:62] > 0).all(), np.flatnonzero(runs.sum(axis=1)[1:62] == 0) + 1
    assert not runs.sum(axis=1)[62:].any()
    assert seqs[3] > 0 and seqs[4] > 0 and runs[:, 3].sum() == seqs[4]      # three equal bytes: literals; four: a literal and a run of 3
    assert (cuts > 0).all(), cuts                              # cut at a chunk's, an eighth's and a block's end


def test_literal_only_and_flat_blocks():
    tr = pc.emu_pngz(pc.built(pc.by_name('nozero'))[2], trace=True)[2]
    assert tr[0]['stored'] == 0 and tr[0]['nlit'] == 257 and not tr[0]['runs'].any()
    tr = pc.emu_pngz(pc.built(pc.by_name('edge-21x780-flat'))[2], trace=True)[2]
    assert tr[0]['stored'] == 0 and tr[0]['nlit'] > 257 and tr[0]['runs'][1, 63] > 0     # whole chunks of one byte: runs of 63
    tr = pc.emu_pngz(pc.built(pc.by_name('adler-ff'))[2], trace=True)[2]
    assert tr[0]['stored'] == 0 and tr[0]['len'] == pc.BLOCK   # a full block of the largest bytes: the per-lane s2 bound


def test_the_limit_case_needs_the_fix_up():
    case = pc.by_name('limit-15')
    rows = pc.built(case)[2]
    first = rows[:pc.BLOCK]
    counts = np.bincount(first, minlength=256).tolist() + [1]                           # + the end-of-block symbol
    assert pc.huffman_depth(counts) > 15
    d = np.flatnonzero(np.diff(first.astype(np.int16)) != 0)
    assert np.diff(np.concatenate([[-1], d, [first.size - 1]])).max() < 4             # no four equal bytes in a row: literals only
    tr = pc.emu_pngz(rows, trace=True)[2]
    assert tr[0]['stored'] == 0 and tr[0]['nlit'] == 257
    assert tr[0]['depth'] > 15 and tr[0]['kraft_changed'] == 1 and tr[0]['max_len'] == 15
