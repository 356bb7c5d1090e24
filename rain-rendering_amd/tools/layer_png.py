"""The rain layer as a file: the numpy statement of the straight-alpha 8-bit RGBA pixel that `main.py --rain_layer`
writes, and of its reader.  csrc/rr_layer.h layer_rgba() is the same arithmetic as an RR_HD function (k_rain_layer<2> calls it on the
device); tests/test_layer_png_host.py holds a g++ build of it equal to encode() byte for byte.

From one pixel's float32 (L_B, L_G, L_R, T):
    a   = 1.0f - T                                        one float32 operation
    A8  = clamp(rint(a * 255.0f), 0, 255)                 float32 multiply, half to even; NaN -> 0
    A8 == 0:  R = G = B = 0
    else      q   = 65025.0 / double(A8)                  one double division (65025 = 255 * 255)
              C_c = clamp(rint(double(L_c) * q), 0, 255)  one double multiply, half to even; NaN -> 0;   c = R, G, B
    file pixel = (C_R, C_G, C_B, A8)
The colour is divided by the QUANTISED alpha, so the reader gets L back from the file's own numbers:
    T' = 1 - A8 / 255          L'_c = A8 C_c / 65025          (double)
and PNG's `over` of the file on x is T' x + L'.

The bound (derived in DESIGN.md 5r).  Wherever 0 <= T <= 1 and 0 <= L_c <= 1 - T, each of |T' - T| and |L'_c - L_c| is at most
BOUND = 1/510 + (2^-17 / 255 + 2^-25): half a code of the alpha, or of the colour scaled by A8 / 255 <= 1, plus the float32 roundings
of a * 255 (half an ulp below 256, brought back to a's scale) and of a = 1 - T (half an ulp below 1).  So
|T' x + L' - (T x + L)| <= 2 BOUND for x in [0, 1]: 1/255 and 1.2e-7."""
import numpy as np

SHIFT_KEYWORD = 'rain-shift'          # the tEXt chunk of a layer file: repr(float) of the frame's mean shift

# |T' - T| and |L'_c - L_c| under the condition; see the module text
BOUND = 1.0 / 510.0 + 2.0 ** -17 / 255.0 + 2.0 ** -25 + 2.0 ** -48          # (2^-48: the double roundings of the reader and of C_c)


def _round_u8(v):
    """clamp(rint(v), 0, 255) with NaN -> 0, as uint8 (fmin(fmax(rint(v), 0), 255): fmax drops the NaN)."""
    with np.errstate(invalid='ignore'):
        r = np.rint(v)
        r = np.where(np.isnan(r), 0.0, r)
        return np.clip(r, 0.0, 255.0).astype(np.uint8)


def encode(layer):
    """[..., 4] float32 (L_B, L_G, L_R, T) -> [..., 4] uint8 (R, G, B, A), straight alpha."""
    layer = np.asarray(layer)
    if layer.dtype != np.float32 or layer.shape[-1] != 4:
        raise ValueError("encode: a float32 array [..., 4] in the order L_B, L_G, L_R, T")
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        a = np.float32(1.0) - layer[..., 3]
        A8 = _round_u8(a * np.float32(255.0))
        q = np.float64(65025.0) / np.where(A8 == 0, 1, A8).astype(np.float64)
        out = np.zeros(layer.shape, np.uint8)
        for c_file, c_layer in ((0, 2), (1, 1), (2, 0)):          # file R, G, B <- layer L_R, L_G, L_B
            C = _round_u8(layer[..., c_layer].astype(np.float64) * q)
            out[..., c_file] = np.where(A8 == 0, 0, C)
        out[..., 3] = A8
    return out


def decode(rgba):
    """[..., 4] uint8 (R, G, B, A) -> (L_B, L_G, L_R, T), four float64 arrays: T' = 1 - A / 255, L'_c = A C_c / 65025."""
    rgba = np.asarray(rgba)
    if rgba.dtype != np.uint8 or rgba.shape[-1] != 4:
        raise ValueError("decode: a uint8 array [..., 4] in the order R, G, B, A")
    A = rgba[..., 3].astype(np.float64)
    L = [A * rgba[..., c].astype(np.float64) / 65025.0 for c in (2, 1, 0)]
    return L[0], L[1], L[2], 1.0 - A / 255.0


def sub_filter(rgba):
    """[H, W, 4] uint8 -> the file's scanlines, [H, 1 + 4 W] uint8: filter type 1 (Sub), each byte minus the byte one pixel to the left."""
    rgba = np.asarray(rgba, np.uint8)
    H, W = rgba.shape[:2]
    rows = np.empty((H, 1 + 4 * W), np.uint8)
    rows[:, 0] = 1
    d = rgba.copy()
    d[:, 1:] = rgba[:, 1:] - rgba[:, :-1]                        # (uint8 arithmetic wraps: the filter's modulo 256)
    rows[:, 1:] = d.reshape(H, 4 * W)
    return rows
