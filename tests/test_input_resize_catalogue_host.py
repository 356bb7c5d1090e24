"""CPU tier of the input-resize catalogue (tests/resize_catalogue.py).  The census: every case reaches the branch of
resize_rows it is listed for, and the catalogue as a whole reaches every item of its list -- decided from predict(), the host
restatement of the launch arithmetic, never from a device result.  The header: the g++ build of csrc/rr_resize.h with
csrc/rr_convert.h's widening (tests/hostemu/resize_emu.cpp) equals resize_linear on the float64 values for every case and kind, as
bit patterns."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import helpers as h
import resize_catalogue as cat

hb = h.hb


def _predict(c, **kw):
    return cat.predict(c.kind, c.H, c.W, c.sH, c.sW, c.offset, **kw)


# the staged widths DESIGN.md 5o records per class: (largest staged source width, first direct one, the limit in columns) at W = 520
EXPECTED_LIMITS = {'bytes interleaved': (6762, 6763, 6646), 'bytes planar': (6740, 6741, 6626), 'float32 planar': (1684, 1685, 1656),
                   'float32 interleaved': (1689, 1690, 1661), 'half planar': (3369, 3370, 3313), 'half interleaved': (3379, 3380, 3323),
                   'uint16 depth': (10143, 10144, 9969), 'float32 depth': (5070, 5071, 4984)}


def test_constants_and_kinds():
    assert cat.RSZ_THREADS == 256 and cat.RSZ_SEG == 512 and cat.RSZ_POOL == 39936
    assert [k.code for k in cat.KINDS.values() if k.image] == list(range(9))                  # RR_RESIZE_* 0 .. 8, none twice
    assert (hb.RR_RESIZE_BGR_U8, hb.RR_RESIZE_RGB_U8_PLANAR, hb.RR_RESIZE_RGB_F32_PLANAR) == (0, 1, 2)      # what existed stays
    header = open(os.path.join(h.ROOT, 'include', 'rainhip.h')).read()                         # the header and the binding agree
    in_header = {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(RR_RESIZE_\w+) = (\d+)', header)}
    assert len(in_header) == 9 and sorted(in_header.values()) == list(range(9))
    assert all(getattr(hb, name) == v for name, v in in_header.items())
    assert len({cat.kind_class(k) for k in cat.KINDS}) == 8
    for kind, k in cat.KINDS.items():
        assert cat.cap(kind) % 16 == 0 and k.EL == (k.el if k.planar or not k.image else 3 * k.el), kind
    for kind in cat.KINDS:
        assert cat.LIMIT_WIDTHS[kind] == EXPECTED_LIMITS[cat.kind_class(kind)][:2] and cat.span_limit(kind) == EXPECTED_LIMITS[cat.kind_class(kind)][2], kind


@pytest.mark.parametrize("name", list(cat.CASES))
def test_census_of_a_case(name):
    """The case reaches what it is for."""
    c = cat.CASES[name]
    k = cat.KINDS[c.kind]
    p = _predict(c)
    segs = p.segments
    assert 1 <= c.H <= 7 and p.grid == ((c.W + 511) // 512, c.H, cat.N) and c.reason
    for s in segs:                                                       # predict() itself: the spans stay inside the source row
        assert 0 <= s.xa <= s.xb < c.sW and s.span == s.xb - s.xa + 1 and s.xs < s.xe <= c.W
    tag = name.split('-')[0]
    if c.group == 'segments':
        assert all(s.staged for s in segs) and segs[1].xa > 0
        if tag == 'seg513':
            assert len(segs) == 2 and segs[1].xe - segs[1].xs == 1 and c.sW == 2 * c.W
        elif tag == 'seg1024':
            assert len(segs) == 2 and segs[1].xe - segs[1].xs == 512 and c.sW == 2 * c.W
        elif tag == 'seg1025':
            assert len(segs) == 3 and segs[2].xe - segs[2].xs == 1 and c.sW == 2 * c.W
        else:
            assert len(segs) == 3 and (c.sW / c.W) % 1 != 0 and (c.sH / c.H) % 1 != 0
    elif c.group == 'limit':
        assert c.W == 520 and len(segs) == 2 and segs[1].staged and segs[1].xe - segs[1].xs == 8 and c.sH % 2 == 1 and c.sH >= 3
        room = cat.cap(c.kind) - 30
        if name.startswith('limit-staged'):
            assert segs[0].staged and segs[0].span == cat.span_limit(c.kind) and segs[0].span * k.EL == room - room % k.EL
        else:
            assert not segs[0].staged and segs[0].span == cat.span_limit(c.kind) + 1 and segs[0].span * k.EL + 30 > cat.cap(c.kind)
        assert len(p.residues) > 1                                       # planes and rows start on differing residues
    elif c.group == 'shapes':
        checks = {'up': len(segs) == 3 and c.sW < c.W and c.sH < c.H,
                  'sw1': c.sW == 1 and len(segs) == 2 and all(s.xa == s.xb == 0 for s in segs),
                  'sw2': c.sW == 2 and len(segs) == 2 and segs[0].xa == 0 and segs[1].xb == 1,
                  'sh1': c.sH == 1 and c.H == 3 and len(segs) == 2,
                  'h1': c.H == 1 and c.sH == 1 and c.sW != c.W and len(segs) == 2,
                  'aniso': (c.H, c.W, c.sH, c.sW) == (7, 700, 3, 1900),
                  'ident': (c.H, c.W) == (c.sH, c.sW) and len(segs) == 3 and segs[2].xe - segs[2].xs == 1}
        assert checks[tag], (name, segs)
    else:
        assert c.group == 'residues' and p.unaligned and c.offset % k.el == 0 and (c.H * c.W) % 2 == 1 and p.tail and len(segs) == 2
        assert {p.stores[(f, 0)] for f in range(cat.N)} == ({'16', '8off'} if k.image else {'pair', 'single'})
        assert p.stores[(0, 0)] != p.stores[(1, 0)] and p.stores[(0, 0)] == p.stores[(2, 0)]      # frames alternate
    # the content holds what the issue lists
    arr, values = cat.case_input(name)
    assert arr.nbytes == cat.N * c.sH * c.sW * (3 if k.image else 1) * k.el and np.isfinite(values).all()
    assert values.shape == ((cat.N, c.sH, c.sW, 3) if k.image else (cat.N, c.sH, c.sW))
    if c.sH * c.sW >= 200:
        top = {('u8', 1): 1.0, ('u16', 2): 65535 / 256}.get((c.kind if not k.image else 'u8', k.el))
        if k.el == 1 or c.kind == 'u16':
            assert values.min() == 0 and values.max() == top
        else:
            tiny, big = {None: (2.0 ** -126, float(np.finfo(np.float32).max)), 'f16': (2.0 ** -14, 65504.0),
                         'bf16': (2.0 ** -126, float(np.float32(2.0 ** 127) * np.float32(1.9921875)))}[k.half]
            a = np.abs(values)
            assert ((a > 0) & (a < tiny)).any() and (a == tiny).any() and (values == big).any() and values.max() == big      # subnormals, normals, the largest
            assert (np.signbit(values) & (values == 0)).any() and ((values == 0) & ~np.signbit(values)).any()                  # -0.0 and 0.0


def test_census_of_the_catalogue():
    """Across all cases every item of the list occurs."""
    preds = {name: _predict(c) for name, c in cat.CASES.items()}
    kinds_two_segments, staged_at_limit, direct_above, mixed = set(), set(), set(), set()
    one_pixel_last, byte_residues, unaligned, image_stores, depth_stores, tails = False, set(), set(), set(), set(), set()
    for name, c in cat.CASES.items():
        p, k = preds[name], cat.KINDS[c.kind]
        if len(p.segments) >= 2:
            kinds_two_segments.add(c.kind)
        for s in p.segments:
            if s.staged and s.span == cat.span_limit(c.kind):
                staged_at_limit.add(cat.kind_class(c.kind))
            if not s.staged and s.span == cat.span_limit(c.kind) + 1:
                direct_above.add(cat.kind_class(c.kind))
        if {s.staged for s in p.segments} == {True, False}:
            mixed.add(c.kind)
        one_pixel_last |= p.segments[-1].xe - p.segments[-1].xs == 1
        if k.el == 1:
            byte_residues |= p.residues
        if p.unaligned:
            unaligned.add(c.kind)
        (image_stores if k.image else depth_stores).update(p.stores.values())
        if p.tail:
            tails.add(k.image)
    assert kinds_two_segments == set(cat.KINDS)
    assert staged_at_limit == direct_above == set(cat.CLASS_NAMES.values())
    assert mixed == set(cat.KINDS)
    assert one_pixel_last and {0, 15} <= byte_residues and unaligned == set(cat.KINDS)
    assert image_stores == {'16', '8off'} and depth_stores == {'pair', 'single'} and tails == {True, False}
    # the old nine cases, for the record: one segment each
    rc = importlib.import_module('resize_cases')
    assert all(w <= 512 for (_, w), _ in list(rc.IMAGE_CASES.values()) + list(rc.DEPTH_CASES.values()))


def test_predict_against_a_brute_force_walk():
    """predict()'s xa / xb are the smallest and largest source column any pixel of the segment touches."""
    for kind, H, W, sH, sW in (('bgr_u8', 2, 520, 3, 6762), ('f32', 3, 1030, 2, 300), ('rgb_f32', 4, 1025, 7, 2049), ('u16', 2, 600, 3, 1)):
        p = cat.predict(kind, H, W, sH, sW)
        for s in p.segments:
            cols = [cat.resize_coord(x, sW, sW / W)[:2] for x in range(s.xs, s.xe)]
            assert s.xa == min(a for a, _ in cols) and s.xb == max(b for _, b in cols), (kind, s)


@pytest.fixture(scope="module")
def emu(built):
    return ctypes.CDLL(importlib.import_module('__graft_entry__').build_emu('resizeemu'))


@pytest.mark.parametrize("name", list(cat.CASES))
def test_header_equals_resize_linear_bit_for_bit(emu, name):
    c = cat.CASES[name]
    k = cat.KINDS[c.kind]
    arr, _ = cat.case_input(name)
    want = cat.case_want(name)
    for f in range(cat.N):
        src = np.ascontiguousarray(arr[f])
        if k.image:
            out = np.full((c.H, c.W, 3), np.nan)
            assert emu.resize_emu_image(h._p(src), k.code, c.sH, c.sW, c.H, c.W, h._p(out)) == 0
        else:
            out = np.full((c.H, c.W), np.nan, np.float32)
            assert emu.resize_emu_depth(h._p(src), k.code, c.sH, c.sW, c.H, c.W, h._p(out)) == 0
        assert out.dtype == want.dtype and not cat.mismatches(out, want[f]), (name, f, cat.mismatches(out, want[f]))
    assert want.min() != want.max()


def test_emu_refuses_a_kind_outside_the_enum(emu):
    src, out = np.zeros(12, np.uint8), np.zeros(3)
    for kind in (-1, 9):
        assert emu.resize_emu_image(h._p(src), kind, 1, 1, 1, 1, h._p(out)) == -1      # RR_E_ARG
