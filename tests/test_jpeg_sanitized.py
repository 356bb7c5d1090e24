"""CPU tier: the library's baseline JPEG reader compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/sanitize/jpeg_fuzz.cpp) and fed every catalogue file (tests/jpeg_cases.py) intact, cut at every length and with single bytes
changed -- through rr_jpeg_info, rr_jpeg_read_record, rr_jpeg_read_bgr8 and rr_io_read_frames_jpeg.  Run as a child process; skipped
where the sanitizer run-times are not installed (a one-line program decides that; the real program then has to build)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as h
import jpeg_cases as jc


def test_jpeg_reader_under_sanitizers(tmp_path):
    from PIL import Image
    src = os.path.join(h.ROOT, 'tests', 'sanitize', 'jpeg_fuzz.cpp')
    exe = str(tmp_path / 'jpeg_fuzz')
    cc = ['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-std=c++17', '-ffp-contract=off',
          '-I' + os.path.join(h.ROOT, 'include'), '-I' + os.path.join(h.ROOT, 'rain-rendering_amd', 'csrc'), src, '-lz', '-lpthread', '-o', exe]
    # the sanitizer run-times are probed for with a program of one line: where that builds, the real program must build too
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    r = subprocess.run(['g++', '-fsanitize=address,undefined', str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no sanitizer build here: " + r.stderr[-300:])
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args, depth = [], {}
    rng = np.random.RandomState(2)
    for (name, W, H, ss, b) in jc.catalogue():
        p = str(tmp_path / (name + '.jpg'))
        with open(p, 'wb') as f:
            f.write(b)
        if (W, H) not in depth:
            depth[(W, H)] = str(tmp_path / ('d%dx%d.png' % (W, H)))
            Image.fromarray(rng.randint(0, 65536, (H, W)).astype(np.uint16)).save(depth[(W, H)])
        args += [p, depth[(W, H)]]
    work = tmp_path / 'work'
    work.mkdir()
    run = subprocess.run([exe, str(work)] + args, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))          # (the buffer pools live until exit by design)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert 'jpeg_fuzz: files %d,' % len(jc.catalogue()) in run.stdout and 'wrong 0' in run.stdout, run.stdout[-600:]
    assert ', tables ' in run.stdout and int(run.stdout.split(', tables ')[1].split(',')[0]) >= 7 * len(jc.catalogue())
    assert int(run.stdout.split('renumbered ')[1].split(',')[0]) == 4 * len(jc.catalogue())
    cuts = int(run.stdout.split('cuts ')[1].split(',')[0])
    assert cuts == sum(len(c[4]) for c in jc.catalogue())                # every length of every file
