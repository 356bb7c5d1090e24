"""CPU tier of the pre-pass pin (tests/prepass_cases.py): the catalogue reaches what it aims at, the bounds stay where their
derivation puts them, the reference is the oracle, and the host build of rr_prepass.h (tests/hostemu) is within the bounds of
the reference for every case -- in the tile form and in the three-kernel form, which agree bit for bit."""
import numpy as np
import pytest

import prepass_cases as pc
import test_prepass_hostemu as tp
from oracle import prepass as op


def _ids(cases):
    return [c.name for c in cases]


def test_reference_is_the_oracle_at_its_own_tap_counts():
    """ref_fog / ref_env_map with 25 and 15 taps against oracle.prepass.fog_rain_layer / generate_env_map, bit for bit, for every
    input of the catalogue that has those counts."""
    n = 0
    for c in pc.catalogue():
        if c.taps != (25, 15):
            continue
        bg, depth = c.inputs
        want = op.fog_rain_layer(pc.widen(bg), pc.metres(depth), c.rain, pc.FNUM, pc.EXPO, pc.GAIN)
        assert np.array_equal(c.rainy, want), c.name
        if c.want_env:
            assert np.array_equal(pc.ref_env_map(c.rainy, pc.env_taps(15)), op.generate_env_map(c.rainy, pc.FOCAL)), c.name
        n += 1
    assert n >= 5 * len(pc.MAP_SIZES)
    assert np.array_equal(pc.fog_taps(25), op.gaussian_kernel(25, 25)) and np.array_equal(pc.env_taps(15), op.gaussian_kernel(15, 0))
    assert np.array_equal(pc.fog_taps(1), [1.0]) and np.array_equal(pc.env_taps(1), [1.0])


def test_catalogue_covers_what_it_names():
    """The sizes against the constants they are aimed at, the types and the tap counts."""
    cat = pc.catalogue()
    for H, W in pc.sizes():
        assert pc.cases_of(H, W), (H, W)
    for H, W in pc.MAP_SIZES:
        assert H >= 2 and W >= 3 and int(((pc.FOCAL * 1000) / 12.7) * W) >= 1
        kinds = {(c.kind, c.f64) for c in pc.cases_of(H, W)}
        assert {('scene', True), ('scene', False), ('sat', True), ('sat', False)} <= kinds
        assert any(c.depth_t == np.uint16 for c in pc.cases_of(H, W))
    assert op.env_geometry(pc.FOCAL, 2, 3)[0] + 2 * (op.env_geometry(pc.FOCAL, 2, 3)[0] // 2) == 5
    assert op.env_geometry(pc.FOCAL, 72, 257)[0] + 2 * (op.env_geometry(pc.FOCAL, 72, 257)[0] // 2) == 393
    # segments of k_fog_tile: (rows per segment, segments)
    segs = {(H, W): (pc.tile_seg_rows(H, W), -(-H // pc.tile_seg_rows(H, W))) for H, W in pc.MAP_SIZES}
    assert segs[(65, 33)] == (72, 1) and 65 % pc.RB == 1
    assert segs[(128, 32)] == (64, 2)
    assert segs[(129, 33)] == (72, 2) and (129 - 72) % pc.RB == 1 and (129 - 72) % pc.VR == 1
    assert segs[(192, 32)] == (64, 3)
    assert 33 % pc.TC == 1 and 257 % pc.FOG_SEG == 1 and 9 < pc.HALF and 5 < pc.HALF and 13 == pc.HALF + 1
    assert {(np.dtype(c.img_t), np.dtype(c.depth_t)) for c in pc.cases_of(*pc.TYPE_SIZE)} >= \
        {(np.dtype(a), np.dtype(b)) for a in pc.IMG_TYPES for b in pc.DEPTH_TYPES}
    for size in pc.TAP_SIZES:
        assert {c.taps for c in pc.cases_of(*size)} == set(pc.TAP_COUNTS)
    assert {c.kind for c in pc.cases_of(*pc.FLAT_SIZE)} >= {'white', 'black'}
    d16 = pc.depth_u16(9, 5)
    assert d16.min() == 0 and d16.max() == 65535
    assert len({c.name for c in cat}) == len(cat)


def test_saturating_and_flat_inputs_reach_their_clamps():
    """From the reference alone: fog values equal to 0 and to 1 and a black map cell, for every saturating case (black and white
    images: the ones they can reach).  The fixed-fraction scene at 40 x 64 and at 72 x 257; the hand-written depth elsewhere."""
    hand = {(H, W): pc.saturating(H, W)[2] for H, W in pc.sizes()}
    assert [s for s, v in hand.items() if not v] == [(72, 257)]
    n = 0
    for c in pc.catalogue():
        got = c.assert_reaches_clamps()
        if c.kind != 'scene':
            assert got is not None
            n += 1
    assert n >= 2 * len(pc.sizes()) + 4
    c = pc.Case(40, 64, 'sat', np.float64, np.float64)
    assert not pc.saturating(40, 64)[2]
    n0, n1, nb = c.assert_reaches_clamps()
    print('40x64 saturating: %d values at 1, %d at 0, %d black cells' % (n1, n0, nb))
    assert (n1, n0, nb) == (4080, 240, 82)
    # and the suite's own scene reaches none of them: that is the gap
    s = pc.Case(40, 64, 'scene', np.float64, np.float64)
    assert not (s.rainy == 0).any() and not (s.rainy == 1).any() and not (s.ref_map == 0).all(axis=-1).any()


def test_bounds_stay_where_their_derivation_puts_them():
    worst64 = worst32 = 0.0
    for c in pc.catalogue():
        if c.f64:
            assert c.bound <= pc.F64_LIMIT, (c.name, c.bound)
            assert c.bound >= 100 * pc.EPS
            worst64 = max(worst64, c.bound)
        else:
            assert pc.ref_expf_error(c.parts).max() < 3.0, c.name       # numpy's SIMD expf: documented to 2.52 ulp
            if c.kind == 'scene' and c.depth_t == np.float32 and c.taps[0] == 25 and c.parts['k3'].max() <= 1.1:      # the suite's scene and blur
                assert c.bound <= pc.SUITE_F32, (c.name, c.bound)
            worst32 = max(worst32, c.bound)
    print('largest float64 bound %.3g, largest float32 bound %.3g' % (worst64, worst32))
    # the count itself, 25 taps at 72 x 257: 10 + 74 + e_ref + 152 (ref_mean_error is e_ref + 2)
    c = pc.Case(72, 257, 'scene', np.float64, np.float64)
    assert pc.mean_chain(72 * 257) == 74
    assert pc.bound_f64_count(c.parts, 25) == 8 + 74 + pc.ref_mean_error(c.parts) + 152
    # the scenes of the suite's own tests
    for H, W, seed in ((96, 160, 3), (96, 160, 4), (375, 1242, 3), (40, 64, 5), (96, 160, 5)):
        bg, depth = pc.h.prepass_scene(H, W, seed, np.float32)
        assert pc.bound_f32(pc.fog_parts(bg, depth, 50, pc.fog_taps(25)), 25) <= pc.SUITE_F32, (H, W, seed)


def _emu(c, tiled, narrow=False):
    bg, depth = c.inputs
    return tp.emu_prepass(bg, depth, c.rain, tiled=tiled, seg_rows=pc.tile_seg_rows(c.H, c.W), narrow=narrow, fog_taps=c.taps[0],
                          env_taps=c.taps[1], want_env=c.want_env)


@pytest.mark.parametrize("c", pc.catalogue(), ids=_ids(pc.catalogue()))
def test_host_build_is_within_the_bounds(c):
    c.assert_reaches_clamps()
    forms = ([1] if c.tiled else []) + [0]
    outs = []
    for tiled in forms:
        rainy, xyY, env8 = _emu(c, tiled)
        rainy32, xyY32, env8_32 = _emu(c, tiled, narrow=True)
        d = c.check_fog(rainy, rainy32)
        if c.want_env:
            c.check_map(rainy, env8, xyY, xyY32, env8_32, expect_ref_map=True)
        outs.append((rainy, xyY, env8))
    print('%s: max |d| %.3g, bound %.3g' % (c.name, d, c.bound))
    if len(outs) == 2:
        for a, b in zip(*outs):
            assert np.array_equal(a, b), (c.name, 'tile form against three-kernel form')
