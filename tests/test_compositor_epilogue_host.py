"""CPU tier: what the compositors' epilogue must look like in the gfx950 assembly, and the census of the frames the GPU tier
runs (tests/compositor_outputs.py).

k_composite32 reads every field of its frame descriptor once, before its first store, as scalar loads.  On this hardware
vmcnt counts stores as well as loads, so a descriptor field fetched again behind a store and waited for with vmcnt(0) makes
the wave wait for that store's acknowledgement: with the fields read through a plain reference the epilogue was eight such
round trips in turn instead of one burst of stores (profiles/compositor_epilogue_cost.md).  scripts/store_drain_scan.py is
the reading aid; this test holds the kernel to the property."""
import importlib.util
import os

import pytest

import helpers as h


def _scan_module():
    spec = importlib.util.spec_from_file_location('store_drain_scan', os.path.join(h.ROOT, 'scripts', 'store_drain_scan.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def kernels():
    """{demangled kernel name: instructions} of the library's device code, cross-compiled once with the product's flags."""
    sds = _scan_module()
    ge = __import__('__graft_entry__')
    assert [f for f in ge.HIP_FLAGS if f != '-shared'] == sds.FLAGS, 'the scan must compile with the flags of build()'
    ks = sds.kernels(sds.assembly())
    short = sds.demangle(ks)
    return sds, {short[n]: body for n, body in ks.items()}


def test_k_composite32_stores_in_one_burst(kernels):
    """From the kernel's first global store to its end: every store of the epilogue, no load of any kind (so none from the
    descriptor) and no s_waitcnt that names vmcnt."""
    sds, ks = kernels
    r = sds.epilogue_report(ks['k_composite32'])
    # the tile's sums (two 16-byte stores), then per pixel of the lane the composite in either form, mask_f64, mask_i32
    assert len(r['stores']) == 2 + 2 * 4, r['stores']
    assert not r['vector_loads'], r['vector_loads']
    assert not r['scalar_loads'], r['scalar_loads']
    assert not r['vmcnt_waits'], r['vmcnt_waits']
    stores, behind = sds.scan(ks['k_composite32'])
    assert stores == len(r['stores']) and not behind, behind


def test_k_composite_reads_no_descriptor_field_behind_a_store(kernels):
    """The float64 compositor's stores come before its tile reduction (an LDS tree with barriers): no load and no wait for one
    behind its first store either."""
    sds, ks = kernels
    r = sds.epilogue_report(ks['k_composite'])
    assert len(r['stores']) >= 5 + 1, r['stores']
    assert not r['vector_loads'] and not r['scalar_loads'], (r['vector_loads'], r['scalar_loads'])
    assert not sds.scan(ks['k_composite'])[1]


def test_the_scan_finds_a_load_behind_a_store():
    """The scan on a text that has the pattern, and on one that has not."""
    sds = _scan_module()
    asm = '\n'.join(['\t.amdhsa_kernel k_a', '\t.end_amdhsa_kernel', 'k_a:', '\tglobal_store_dword v[0:1], v2, off',
                     '\tglobal_load_dwordx2 v[0:1], v2, s[30:31] offset:56', '\ts_waitcnt vmcnt(0)', '\tglobal_store_dword v[0:1], v2, off',
                     '\ts_endpgm', '.Lfunc_end0:',
                     '\t.amdhsa_kernel k_b', '\t.end_amdhsa_kernel', 'k_b:', '\tglobal_load_dword v2, v[0:1], off', '\ts_waitcnt vmcnt(0)',
                     '\ts_barrier', '\tglobal_store_dword v[0:1], v2, off', '\tglobal_store_dword v[0:1], v2, off offset:4', '\ts_endpgm', '.Lfunc_end1:'])
    ks = sds.kernels(asm)
    assert sorted(ks) == ['k_a', 'k_b']
    stores, behind = sds.scan(ks['k_a'])
    assert stores == 2 and [(b[0], b[2]) for b in behind] == [(5, 6)]
    r = sds.epilogue_report(ks['k_a'])
    assert len(r['vector_loads']) == 1 and len(r['vmcnt_waits']) == 1
    assert sds.scan(ks['k_b']) == (2, [])
    r = sds.epilogue_report(ks['k_b'])
    assert len(r['stores']) == 2 and not r['vector_loads'] and not r['vmcnt_waits']
    assert [s for _, s in sds.tail(ks['k_b'])] == ['global_store_dword v[0:1], v2, off', 'global_store_dword v[0:1], v2, off offset:4', 's_endpgm']


def test_census_of_the_output_frames(built, tmp_path):
    """Dead second pixels, dead waves, both seams, every combination of optional outputs, the code-65535 pixel: all reached."""
    import compositor_cases as cc
    import compositor_outputs as co
    tpl = cc.Templates(tmp_path / 'tpl')
    c, tables, bgs = co.build(tmp_path / 'case', tpl)
    n = co.census(c, tables, bgs, co.references(c, tables, bgs))
    # 16 x 32 tiles on 24 x 40: tile row 0 is all live (24 x 16 lanes), in tile row 1 the upper waves' 24 x 8 lanes own one pixel
    assert n['both_live'] == 24 * 16 and n['first_only'] == 24 * 8 and n['both_dead'] == 4 * 256 - 24 * 24
