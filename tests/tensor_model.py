"""The tensor decode's yardstick (numpy, no GPU): the bit patterns himg_hip_decode_tensor_device must
write for a uint8 H x W x C picture and a descriptor.  Element (c, i, j) is
cvt(fma_f32((float)p, scale[c], bias[c])) of byte p = img[i, j, c]: per output channel a 256-entry
table of bit patterns, indexed with the picture.

The table: d = float64(v) * float64(scale) + float64(bias).  The product is exact in double (8 x 24
significant bits), and the sum is exact for every descriptor the tests use -- asserted with
fractions.Fraction for every entry -- so np.float32(d) is the single rounding a fused multiply-add
performs.  F16 is np.float16 of that binary32 value (round to nearest even); BF16 is round to
nearest even on the binary32 bits, in integer arithmetic."""
from fractions import Fraction

import numpy as np

import himg_amd

F32, F16, BF16 = himg_amd.HIMG_DT_F32, himg_amd.HIMG_DT_F16, himg_amd.HIMG_DT_BF16
DTYPES = (F32, F16, BF16)
ELEM = {F32: 4, F16: 2, BF16: 2}
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def identity(dtype, co):
    return himg_amd.tensor_desc(dtype, co)


def imagenet(dtype, co):
    """ImageNet mean / std on the colour channels; a fourth channel (alpha) maps to 0..1."""
    n = min(max(co, 0), 4)
    mean = (IMAGENET_MEAN + (0.0,))[:n]
    std = (IMAGENET_STD + (1.0,))[:n]
    return himg_amd.tensor_desc(dtype, co, mean=mean, std=std)


def mix(dtype, co):
    """A negative scale and powers of two: 128 - v / 2, 2 v - 1 (509 needs nine significant bits:
    bfloat16 rounds), v / 128 + 1 / 2, v / 256 - 1 / 4 (zero at v = 64)."""
    n = min(max(co, 0), 4)
    return himg_amd.tensor_desc(dtype, co, scale=(-0.5, 2.0, 0.0078125, 0.00390625)[:n],
                                bias=(128.0, -1.0, 0.5, -0.25)[:n])


DESCS = {"identity": identity, "imagenet": imagenet, "mix": mix}


def f32_table(scale, bias):
    """fma_f32(v, scale, bias) for v = 0..255 as float32; scale and bias are float32 values."""
    s, b = float(np.float32(scale)), float(np.float32(bias))
    out = np.empty(256, np.float32)
    for v in range(256):
        d = float(v) * s + b
        assert Fraction(d) == Fraction(v) * Fraction(s) + Fraction(b), (v, scale, bias)   # d is the exact real value
        out[v] = np.float32(d)
    return out


def bf16_bits(x):
    """Round to nearest even from binary32 to bfloat16, on the bits (finite values)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_bits(x32, dtype):
    x32 = np.ascontiguousarray(x32, np.float32)
    if dtype == F32:
        return x32.view(np.uint32).copy()
    if dtype == F16:
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).view(np.uint16).copy()
    return bf16_bits(x32)


def tables(desc):
    """[Co][256] bit patterns of the descriptor's type."""
    return np.stack([to_bits(f32_table(desc.scale[c], desc.bias[c]), desc.dtype) for c in range(desc.out_channels)])


def expected(img, desc):
    """The bit patterns of the [Co][H][W] tensor of picture img (H x W x C uint8)."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    t = tables(desc)
    return np.stack([t[c][img[:, :, c]] for c in range(desc.out_channels)])
