"""CPU tier: the driver on trees of JPEG frames, around a stand-in for the GPU context that records what reaches the pipeline.  A
baseline .jpg / .jpeg tree takes the batch-native route and hands over coefficient records whose pixels (the numpy statement of
tests/jpeg_cases.py on the record) are PIL's decode of the files; a progressive tree takes the general route with PIL's pixels, and
under --device_particles the error names the file and the reader's reason."""
import importlib
import os
import sys

import numpy as np
import pytest
from PIL import Image

import helpers as h
import jpeg_cases as jc
import test_pngrows_host as tr

sys.path.insert(0, os.path.join(h.ROOT, 'scripts'))
import driver_host_only as dho                                     # noqa: E402  (the stand-in context lives with the script)

hb = h.hb
main_mod = importlib.import_module('rain-rendering_amd.main')
H, W = 48, 80


def _inputs(fr):
    if fr.get('bg_jpeg') is not None:
        rec = np.array(fr['bg_jpeg'])
        head = rec[:32].view(np.int32)
        assert head[0] == 0x314a5252 and tuple(fr['shape']) == (head[2], head[1])
        n = int(head[4])
        bg = jc.pixels_of(int(head[1]), int(head[2]), int(head[3]), rec[32:32 + 128 * n].view(np.uint16).reshape(n, 64),
                          rec[416:].view(np.int16).reshape(-1, 64))
        return 'record', bg, tr._unfilter(np.ascontiguousarray(fr['depth_png_rows']), head[2], head[1], 2)
    if fr.get('bg_png_rows') is not None:
        return 'rows', None, None
    return 'pixels', (fr['bg_u8'] if fr.get('bg_u8') is not None else fr['bg']), fr['depth']


class RecordingContext(dho.HostOnlyContext):
    log = None

    def pipeline_submit_prepared(self, slot, prep, n=None):
        for k in range(prep.n if n is None else n):
            kind, bg, depth = _inputs(prep.frames[k])
            RecordingContext.log.append(dict(kind=kind, bg=np.array(bg), depth=np.array(depth), sim=prep.frames[k].get('sim') is not None))
        super().pipeline_submit_prepared(slot, prep, n)

    def pipeline_prepare(self, frames, outs):
        p = super().pipeline_prepare(frames, outs)
        p.set_drop_count = lambda k, n_: None
        return p

    def pipeline_wait(self, slot):
        prep, n = self.batches.pop(slot, (None, 0))
        for k in range(n):
            o = prep.outs[k]
            rows = np.zeros((H, 1 + 4 * W), np.uint8)
            rows[:, 1:] = 255
            o['rainy_png'][...] = rows.ravel()
            o['mask_png'][...] = rows.ravel()
            o['status'][...] = 0
            if o.get('n_drops') is not None:
                o['n_drops'][0] = 7
        return True


def _tree(tmp, n, suffixes, **enc):
    """The synthetic dataset with its image files re-encoded as JPEG: {frame index: (path, PIL's decode B G R)}."""
    src = os.path.join(tmp, 'source')
    img_dir, dep_dir = h.synthetic.write_dataset(src, 'kitti', os.path.join('data_object', 'training'), n, H, W)
    h.synthetic.write_streak_db(os.path.join(tmp, 'rainstreakdb'))
    xml = os.path.join(tmp, 'particles', 'kitti', 'data_object', 'rain', '5mm', 'sim_camera0.xml')
    h.synthetic.write_particles_xml(xml, h.synthetic.simulate_particles(2, 200, W, H))
    out = {}
    for i in range(n):
        png = os.path.join(img_dir, '%06d.png' % i)
        rgb = np.array(Image.open(png).convert('RGB'))
        os.remove(png)
        p = os.path.join(img_dir, '%06d%s' % (i, suffixes[i % len(suffixes)]))
        b = jc.encode(rgb, **enc)
        with open(p, 'wb') as f:
            f.write(b)
        out[i] = (p, jc.pil_bgr(b))
    return src, out, dep_dir


def _run(tmp, src, monkeypatch, extra=()):
    monkeypatch.setenv('RAIN_BATCH', '3')
    monkeypatch.setattr(hb, 'RainHip', RecordingContext)
    RecordingContext.log = []
    argv = ['--dataset', 'kitti', '-k', src, '-d', src, '-r', os.path.join(tmp, 'particles'), '-sd', os.path.join(tmp, 'rainstreakdb'),
            '-i', '5', '--output', os.path.join(tmp, 'out'), '--noverbose'] + list(extra)
    gen = main_mod.main(argv)
    return gen, RecordingContext.log, os.path.join(tmp, 'out', 'kitti', 'data_object', 'training', 'rain', '5mm')


@pytest.mark.parametrize("extra", [(), ('--device_particles',)])
def test_baseline_jpeg_tree_takes_the_native_route(tmp_path, built, monkeypatch, extra):
    tmp = str(tmp_path)
    n = 7
    src, frames, dep_dir = _tree(tmp, n, ('.jpg', '.jpeg', '.JPG'), quality=92, sampling=jc.S420)
    gen, log, out = _run(tmp, src, monkeypatch, extra)
    assert gen.timing[0].get('route') == 'native' and len(log) == n == len(gen.stats)
    assert all(fr['kind'] == 'record' for fr in log) and all(fr['sim'] == bool(extra) for fr in log)
    got = {fr['bg'].tobytes(): fr for fr in log}
    for i, (p, bgr) in frames.items():
        fr = got[bgr.tobytes()]                                     # the record's pixels are PIL's decode of the file
        assert np.array_equal(fr['depth'], np.array(Image.open(os.path.join(dep_dir, '%06d.png' % i))))
        for folder in ('rainy_image', 'rain_mask'):                 # .jpg, .jpeg and .JPG lose their whole suffix
            assert os.path.exists(os.path.join(out, folder, '%06d.png' % i)), (folder, i)
    assert sorted(os.listdir(os.path.join(out, 'rainy_image'))) == ['%06d.png' % i for i in range(n)]


def test_a_file_the_reader_refuses_mid_run_is_skipped_like_a_bad_depth_map(tmp_path, built, monkeypatch, capsys):
    tmp = str(tmp_path)
    n = 6
    src, frames, dep_dir = _tree(tmp, n, ('.jpg',), quality=92, sampling=jc.S420)
    rgb = frames[3][1][..., ::-1]
    with open(frames[3][0], 'wb') as f:
        f.write(jc.encode(np.ascontiguousarray(rgb), progressive=True))
    with open(os.path.join(dep_dir, '%06d.png' % 1), 'wb') as f:
        f.write(b'not a png')
    with open(frames[2][0], 'wb') as f:                             # a grey file among 4:2:0 ones: a record that fits, of another sampling
        f.write(jc.encode(np.ascontiguousarray(frames[2][1][..., 1])))
    gen, log, out = _run(tmp, src, monkeypatch)
    assert gen.timing[0].get('route') == 'native' and len(log) == n - 3
    assert {fr['bg'].tobytes() for fr in log} == {frames[i][1].tobytes() for i in (0, 4, 5)}
    assert sorted(os.listdir(os.path.join(out, 'rainy_image'))) == ['%06d.png' % i for i in (0, 4, 5)]
    said = capsys.readouterr().out
    assert '000003.jpg' in said and 'progressive' in said and '000002.jpg' in said and 'sampling' in said and '000001.jpg' in said


def test_progressive_tree_takes_the_general_route(tmp_path, built, monkeypatch):
    tmp = str(tmp_path)
    n = 4
    src, frames, dep_dir = _tree(tmp, n, ('.jpg',), quality=92, sampling=jc.S420, progressive=True)
    gen, log, out = _run(tmp, src, monkeypatch)
    assert gen.timing[0].get('route') != 'native' and len(log) == n
    assert all(fr['kind'] == 'pixels' for fr in log)
    assert {fr['bg'].tobytes() for fr in log} == {bgr.tobytes() for _, bgr in frames.values()}
    with pytest.raises(NotImplementedError, match=r'000000\.jpg: jpeg: progressive'):
        _run(tmp, src, monkeypatch, ('--device_particles',))


def test_cap_batch_counts_the_record_block(built):
    gen = importlib.import_module('rain-rendering_amd.common.generator').Generator.__new__(
        importlib.import_module('rain-rendering_amd.common.generator').Generator)
    os.environ.pop('LOCAL_WORLD_SIZE', None)
    rb = hb.jpeg_record_bytes(1600, 900, jc.S420)
    assert rb == 416 + 128 * (100 * 57 * 4 + 2 * 100 * 57)                 # 57 MCU rows of 16: 900 pads to 912
    old = os.environ.get('RAIN_PINNED_MB')
    os.environ['RAIN_PINNED_MB'] = '1024'
    try:
        plain = gen._cap_batch(10 ** 6, 900, 1600, [], None)
        jpeg = gen._cap_batch(10 ** 6, 900, 1600, [], None, jpeg_bytes=rb)
    finally:
        os.environ.pop('RAIN_PINNED_MB') if old is None else os.environ.__setitem__('RAIN_PINNED_MB', old)
    per = lambda b: 1024 * 2 ** 20 // (hb.RR_PIPE_SLOTS * b)
    base = 900 * 1600 * 15 + 2 * 900 + 1024 * 116
    assert plain == per(base) and jpeg == per(base + rb + 900 * (1 + 2 * 1600) - 900 * 1600 * 7)
