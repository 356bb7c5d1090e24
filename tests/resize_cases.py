"""The cases of the render-scale resize of the inputs (csrc/rr_resize.h; k_resize_in / k_resize_depth), shared by
tests/test_input_resize_host.py (the g++ build of the header and the host loader against numpy) and tests/test_gpu_input_resize.py
(the kernels against numpy).  Destination <- source; n = 3 frames per case, seeded noise that holds 0, 255 and 65535.  The reference
of every comparison is common/imgops.py resize_linear (the cv2.resize restatement tests/test_driver_host.py pins), bit for bit."""
import importlib

import numpy as np

imgops = importlib.import_module('rain-rendering_amd.common.imgops')

N = 3
# name: (destination H, W), (source H, W)
IMAGE_CASES = {'a': ((48, 80), (96, 160)),       # every weight 0.5
               'b': ((48, 80), (97, 161)),       # weights differ per row and column; source rows of 483 bytes, unaligned
               'c': ((32, 53), (96, 160)),       # scale 3; odd W: the pixel-pair tail
               'd': ((48, 81), (48, 81))}        # identity
# one more than the table of DESIGN 5o: a 512-pixel segment whose source span does not fit its share of the LDS pool reads global memory directly
IMAGE_CASES['w'] = ((2, 512), (3, 7168))         # scale 14: 21 KB of interleaved bytes, 7 KB per plane, 28 KB per float plane
DEPTH_CASES = {'e': ((48, 80), (24, 40)),        # up-sampling: floor(f) < 0 at index 0 and the clamp at s - 1
               'f': ((48, 80), (96, 160)),       # down-sampling by 2
               'g': ((48, 80), (97, 161)),       # fractional ratio
               'h': ((48, 80), (48, 80))}        # identity
DEPTH_CASES['x'] = ((2, 512), (3, 10240))        # scale 20: 20 KB of samples, 40 KB of float32 metres per segment: the direct path
IMAGE_KINDS = ('bgr_u8', 'rgb_u8_planar', 'rgb_f32_planar_bytes', 'rgb_f32_planar')
DEPTH_KINDS = ('u16', 'f32')

_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def image_bytes(case):
    """[N, sH, sW, 3] uint8 B G R of an image case."""
    key = ('img', case)
    if key not in _cache:
        sH, sW = IMAGE_CASES[case][1]
        rng = np.random.RandomState(7000 + ord(case))
        a = rng.randint(0, 256, (N, sH, sW, 3)).astype(np.uint8)
        a[:, 0, 0], a[:, -1, -1], a[:, 1, 2], a[:, 2, 1] = 0, 255, 255, 0
        _cache[key] = _frozen(a)
    return _cache[key]


def image_input(case, kind):
    """(array handed to the stage, planar?, the [N, sH, sW, 3] B G R values as float64 that resize_linear takes)."""
    key = ('in', case, kind)
    if key not in _cache:
        bgr = image_bytes(case)
        if kind == 'bgr_u8':
            v = (bgr, False, bgr / 255.0)
        elif kind == 'rgb_u8_planar':
            v = (np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)), True, bgr / 255.0)
        else:
            if kind == 'rgb_f32_planar_bytes':               # byte / 255 as float32: what ToTensor makes
                f = (bgr.astype(np.float32) / np.float32(255.0)).astype(np.float32)
            else:                                            # arbitrary floats in [0, 1]
                f = np.random.RandomState(7100 + ord(case)).uniform(0, 1, bgr.shape).astype(np.float32)
                f[:, 0, 0], f[:, -1, -1] = 0.0, 1.0
            v = (np.ascontiguousarray(f[..., ::-1].transpose(0, 3, 1, 2)), True, f.astype(np.float64))
        _cache[key] = tuple(_frozen(a) if isinstance(a, np.ndarray) else a for a in v)
    return _cache[key]


def image_want(case, kind):
    """[N, H, W, 3] float64 B G R: resize_linear of every frame."""
    key = ('want', case, kind)
    if key not in _cache:
        (H, W), _ = IMAGE_CASES[case]
        _cache[key] = _frozen(np.stack([imgops.resize_linear(f, W, H) for f in image_input(case, kind)[2]]))
    return _cache[key]


def depth_input(case, kind):
    """[N, dH, dW] uint16 samples, or their metres (sample / 256 in float32) plus arbitrary float32 metres in frame 2."""
    key = ('dep', case, kind)
    if key not in _cache:
        sH, sW = DEPTH_CASES[case][1]
        rng = np.random.RandomState(7200 + ord(case))
        d = rng.randint(0, 65536, (N, sH, sW)).astype(np.uint16)
        d[:, 0, 0], d[:, -1, -1], d[:, 1, 1] = 0, 65535, 65535
        if kind == 'f32':
            d = d.astype(np.float32) / np.float32(256.0)
            d[2] = rng.uniform(0.5, 300.0, (sH, sW)).astype(np.float32)
        _cache[key] = _frozen(d)
    return _cache[key]


def scene_depth(case):
    """The uint16 samples of a depth case for a whole-pipeline run: nothing nearer than 2 m (the fog layer divides by the depth;
    65535 stays in)."""
    return _frozen(np.maximum(depth_input(case, 'u16'), np.uint16(512)))


def depth_metres(d):
    return d.astype(np.float32) / np.float32(256.0) if d.dtype == np.uint16 else d


def depth_want(case, kind):
    """[N, H, W] float32: cv2.resize keeps float32 -- resize_linear in float64, rounded once (generator.py:377-381)."""
    key = ('dwant', case, kind)
    if key not in _cache:
        (H, W), _ = DEPTH_CASES[case]
        m = depth_metres(depth_input(case, kind))
        _cache[key] = _frozen(np.stack([imgops.resize_linear(f, W, H).astype(np.float32) for f in m]))
    return _cache[key]
