"""The frames of tests/test_gpu_compositor_outputs.py and their census: the smallest call that reaches every branch of the
compositors' epilogue (rainhip.hip k_composite32 / k_composite read the frame's descriptor once, before their first store).

Three frames of 24 x 40 (W x H) in ONE call, made as tests/compositor_cases.py makes its frames:
  * the second tile column has 8 live columns, the second tile row of k_composite32 (16 x 32 tiles) 8 live rows: there a
    lane's first pixel is live and its second is not, and the lower two waves own no pixel at all;
  * drops across the tile seams x = 16 and y = 32, and one inside the lower right tile;
  * the frames differ in the outputs they ask for, where the C interface allows a null (rr_render_frames_device: mask_f64
    and mask_i32): frame 0 mask_f64 only, frame 1 mask_i32 only, frame 2 both -- and in their drop tables, so an output
    pointer taken from another frame's descriptor puts another frame's values into the array;
  * frame 2 has one input pixel outside [0, 1] that no drop and no drop's pad reaches: code 65535 of the 16-bit composite.
census() checks all of that from the frame descriptions, on the host."""
import numpy as np

import compositor_cases as cc
import helpers as h

W, H = 24, 40
WILD_PX = (2, 21)                          # (y, x): upper tile row, second tile column
WILD_VALUE = (1.5, -0.5, 2.0)
# which optional outputs a frame asks for: (mask_f64, mask_i32)
WANTS = ((True, False), (False, True), (True, True))


def _table(c, rows):
    first = len(c.rows)
    for name, tname, x, y, shift in rows:
        c.add(name, tname, x, y, shift=shift)
    return list(range(first, len(c.rows)))


def build(tmp, tpl):
    """(case, tables, backgrounds): the Case holds the drops of both tables, tables[k] the indices frame k uses."""
    c = cc.Case('outputs', tmp, tpl, H, W)
    a = _table(c, (('a_seam_x', 'v8', 14, 10, -4.0), ('a_seam_y', 'v12', 5, 26, 6.0), ('a_seam_xy', 'big', 12, 27, -2.0),
                   ('a_lower_right', 'v6', 18, 33, 4.0), ('a_lower_left', 'v3', 3, 36, -6.0), ('a_over', 'v3', 14, 12, 6.0),
                   ('a_last_rows', 'v5', 20, 35, -4.0)))
    b = _table(c, (('b_seam_x', 'v6', 15, 4, 6.0), ('b_seam_y', 'v20', 19, 22, -4.0), ('b_lower', 'v7', 9, 33, -2.0),
                   ('b_upper', 'o9', 2, 3, 4.0), ('b_corner', 'v2', 22, 38, -6.0)))
    c.finish()
    wild = c.bg.copy()
    wild[WILD_PX] = WILD_VALUE
    return c, (a, b, a), (c.bg, c.bg, wild)


def references(c, tables, bgs):
    """The host emulation of every frame."""
    return [c.emu(c.drops[idx], bg=bg) for idx, bg in zip(tables, bgs)]


def lanes(geom):
    """Per lane of every workgroup of the frame: (first pixel live, second pixel live); the second is None where a lane has one."""
    out = []
    for tyi in range(-(-H // geom['th'])):
        for txi in range(-(-W // geom['tw'])):
            for wave in range(4):
                for lane in range(64):
                    px = txi * geom['tw'] + geom['sx'] * (wave & 1) + (lane & 7)
                    py0 = tyi * geom['th'] + geom['sy'] * (wave >> 1) + (lane >> 3)
                    py1 = None if geom['second'] is None else py0 + geom['second']
                    out.append((px < W and py0 < H, None if py1 is None else (px < W and py1 < H)))
    return out


def census(c, tables, bgs, refs):
    """Every case the test is about is reached; returns the counts."""
    n = {}
    assert W - cc.TILE == 8 and H - cc.TILE32_H == 8
    l32 = lanes(cc.GEOM32)
    n['both_live'] = sum(1 for a, b in l32 if a and b)
    n['first_only'] = sum(1 for a, b in l32 if a and not b)
    n['both_dead'] = sum(1 for a, b in l32 if not a and not b)
    n['second_only'] = sum(1 for a, b in l32 if not a and b)
    assert n['both_live'] and n['first_only'] and n['both_dead'] and not n['second_only'], n
    assert n['both_live'] * 2 + n['first_only'] == W * H
    l64 = lanes(cc.GEOM64)
    n['dead_f64'] = sum(1 for a, _ in l64 if not a)
    assert n['dead_f64'] and sum(1 for a, _ in l64 if a) == W * H
    # the outputs a frame may leave out: each combination but "none", each once
    assert sorted(WANTS) == [(False, True), (True, False), (True, True)] and len(tables) == len(WANTS) == len(bgs)
    n['null_outputs'] = sum(1 for w in WANTS for x in w if not x)
    assert n['null_outputs'] == 2
    # the tables differ, and every drop of them is rendered
    assert tables[0] != tables[1] and tables[2] == tables[0]
    assert not np.array_equal(refs[0]['mask'], refs[1]['mask'])
    for k, (idx, ref) in enumerate(zip(tables, refs)):
        keep, boxes = cc.listed_drops(c.scene, c.drops[idx], ref['status'])
        assert len(keep) == len(idx), (k, keep)
        assert any(b[0] < cc.TILE < b[2] for b in boxes) and any(b[1] < cc.TILE32_H < b[3] for b in boxes), (k, boxes)
        lower = [b for b in boxes if b[1] >= cc.TILE32_H]
        assert lower and any(b[0] >= cc.TILE for b in lower), (k, boxes)
        rows = np.nonzero(ref['mask'].any(axis=1))[0]
        assert rows.max() >= cc.TILE32_H and (ref['mask'][cc.TILE32_H:, cc.TILE:] > 0).any(), k
        assert (ref['mask'] == 0).any()                      # pixels no drop reaches: the poison must go there too
    n['seam_drops'] = sum(1 for b in cc.listed_drops(c.scene, c.drops[tables[0]], refs[0]['status'])[1] if b[0] < cc.TILE < b[2] or b[1] < cc.TILE32_H < b[3])
    # the pixel outside [0, 1]: in one frame only, outside every drop's padded rectangle (the host build clips under a pad, as
    # the reference does; the library only with RR_OPT_WILD_PIXELS), so it leaves the compositor as code 65535
    y, x = WILD_PX
    wild = [k for k, bg in enumerate(bgs) if not ((bg >= 0.0) & (bg <= 1.0)).all()]
    assert wild == [2] and ((bgs[2] < 0.0) | (bgs[2] > 1.0)).any(axis=2).sum() == 1
    plans, sizes = h.emu_plan(c.scene, c.drops[tables[2]])
    for p, s in zip(plans, sizes):
        assert s > 0
        assert not (p['vis_x0'] <= x < p['vis_x0'] + p['vis_w'] and p['vis_y0'] <= y < p['vis_y0'] + p['vis_h']), p
    assert refs[2]['mask'][y, x] == 0.0 and tuple(refs[2]['rainy_bg'][y, x]) == WILD_VALUE
    n['code_65535_pixels'] = 1
    return n
