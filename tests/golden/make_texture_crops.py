"""tests/golden/textures/*.png: crops of the PNG textures the reference's scenes name
(scenes/textures/*.png, 2048x2048 RGB, 1.3 MB each: too large to commit), for
tests/test_png_decode.py::test_reference_textures_match_pillow.

A crop keeps what a decoder sees of the original file: the same colour type and bit depth, every
ancillary chunk copied verbatim (pHYs, the iTXt XMP packet), every row filtered with the filter type
the original file uses for that row, and the zlib stream split into IDAT chunks of the original's
chunk size.  Only the pixels outside the window are dropped.

    python tests/golden/make_texture_crops.py <reference checkout>/scenes/textures
"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
X0, Y0, W, H = 701, 533, 509, 383      # odd offset and size, inside every 2048x2048 texture


def chunks(data):
    pos = 8
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        yield tag, data[pos + 8:pos + 8 + n]
        pos += 12 + n


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)


def unfilter(raw, w, h, bpp):
    """-> (pixels h x w*bpp uint8, filter type per row)"""
    stride = w * bpp
    out = np.zeros((h, stride), np.uint8)
    types = []
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int32)
        types.append(ft)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:                      # left-dependent filters: serial along the row (plain lists are faster)
            ln, pv, cu = line.tolist(), prev.tolist(), [0] * stride
            for i in range(stride):
                a = cu[i - bpp] if i >= bpp else 0
                b = pv[i]
                c = pv[i - bpp] if i >= bpp else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cu[i] = (ln[i] + p) & 255
            cur = np.array(cu, np.int32)
        out[y] = cur
        prev = cur
    return out, types


def refilter(px, types, bpp):
    h, stride = px.shape
    raw = bytearray()
    prev = np.zeros(stride, np.int32)
    zero = np.zeros(bpp, np.int32)
    for y in range(h):
        cur = px[y].astype(np.int32)
        a = np.concatenate([zero, cur[:-bpp]])
        c = np.concatenate([zero, prev[:-bpp]])
        ft = types[y]
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - a
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((a + prev) >> 1)
        else:
            pa, pb, pc = abs(prev - c), abs(a - c), abs(a + prev - 2 * c)
            f = cur - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        raw += bytes([ft]) + bytes((f & 255).astype(np.uint8))
        prev = cur
    return bytes(raw)


def crop(src, dst):
    data = open(src, "rb").read()
    parts = list(chunks(data))
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", parts[0][1])
    assert (depth, ctype, lace) == (8, 2, 0), (depth, ctype, lace)
    idat = [b for t, b in parts if t == b"IDAT"]
    px, types = unfilter(zlib.decompress(b"".join(idat)), w, Y0 + H, 3)     # the rows down to the window's last
    win = np.ascontiguousarray(px[Y0:Y0 + H, 3 * X0:3 * (X0 + W)])
    z = zlib.compress(refilter(win, types[Y0:Y0 + H], 3), 9)
    step = max(len(b) for b in idat)
    out = data[:8] + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, comp, filt, lace))
    out += b"".join(chunk(t, b) for t, b in parts[1:] if t not in (b"IDAT", b"IEND"))
    out += b"".join(chunk(b"IDAT", z[i:i + step]) for i in range(0, len(z), step)) + chunk(b"IEND", b"")
    with open(dst, "wb") as f:
        f.write(out)
    print(dst, len(out), "bytes; filters used:", sorted(set(types[Y0:Y0 + H])), "IDAT chunk", step)


if __name__ == "__main__":
    src = sys.argv[1]
    os.makedirs(os.path.join(HERE, "textures"), exist_ok=True)
    for name in sorted(os.listdir(src)):
        if name.endswith(".png"):
            crop(os.path.join(src, name), os.path.join(HERE, "textures", name))
