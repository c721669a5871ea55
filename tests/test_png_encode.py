"""PNG encoding on the device (engine.op_png_encode, csrc/png_encode.hip + csrc/png_chunk.h): every stream is a valid zlib stream of
the scanlines filtered by the min-sum-of-absolute-values heuristic (restated below in numpy and pinned to Pillow), the container
around it opens in Pillow to the input, nothing is written past the stream, and the files stay within the size caps.

The encoder's body is one text for the HIP kernels and for a host-thread build (tests/png_host/png_host.cpp); the cases run on both,
the host build without a GPU."""
import io
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from swapnet_amd import _C, engine
from swapnet_amd.util.png import png_container
from tests import backends

REPO = backends.REPO
SENTINEL = 0xA5


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img):
    """PNG filtering of an (H,W,3) uint8 image, bpp 3, per row the type with the smallest sum of min(b, 256 - b); ties to the lower
    type.  Returns (H, 1 + 3W) uint8: type byte, then the row."""
    h, w, _ = img.shape
    raw = img.reshape(h, 3 * w).astype(np.int64)
    out = np.zeros((h, 1 + 3 * w), np.uint8)
    for y in range(h):
        x = raw[y]
        up = raw[y - 1] if y else np.zeros_like(x)
        left = np.concatenate([np.zeros(3, np.int64), x[:-3]])
        upleft = np.concatenate([np.zeros(3, np.int64), up[:-3]])
        cands = [x, x - left, x - up, x - (left + up) // 2, x - _paeth(left, up, upleft)]
        cands = [c & 255 for c in cands]
        costs = [int(np.minimum(c, 256 - c).sum()) for c in cands]
        t = int(np.argmin(costs))                      # (argmin: the first minimum)
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out


def unfilter(filtered, h, w):
    f = np.frombuffer(bytes(filtered), np.uint8).reshape(h, 1 + 3 * w)
    raw = np.zeros((h, 3 * w), np.int64)
    for y in range(h):
        t, row = int(f[y, 0]), f[y, 1:].astype(np.int64)
        up = raw[y - 1] if y else np.zeros(3 * w, np.int64)
        assert 0 <= t <= 4
        if t == 0:
            raw[y] = row
        elif t == 2:
            raw[y] = (row + up) & 255
        else:
            for i in range(3 * w):
                a = raw[y, i - 3] if i >= 3 else 0
                c = up[i - 3] if i >= 3 else 0
                pred = a if t == 1 else ((a + up[i]) // 2 if t == 3 else int(_paeth(np.int64(a), up[i], np.int64(c))))
                raw[y, i] = (row[i] + pred) & 255
    return raw.astype(np.uint8).reshape(h, w, 3)


def idat_of(png_bytes):
    """The concatenated IDAT payload of a PNG file (CRCs checked)."""
    assert png_bytes[:8] == b"\x89PNG\r\n\x1a\n"
    pos, data = 8, b""
    while pos < len(png_bytes):
        n, kind = struct.unpack(">I4s", png_bytes[pos:pos + 8])
        body = png_bytes[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", png_bytes[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IDAT":
            data += body
        pos += 12 + n
    return data


def first_block_header(stream):
    """(BTYPE, literal / length code lengths, distance code lengths, code-length symbols used) of the first deflate block."""
    bits = int.from_bytes(stream[2:], "little")
    pos = [0]

    def take(n):
        v = (bits >> pos[0]) & ((1 << n) - 1)
        pos[0] += n
        return v

    take(1)
    btype = take(2)
    if btype != 2:
        return btype, None, None, None
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = take(3)
    code, table = 0, {}
    for length in range(1, 8):                         # canonical code-length code, keyed by (length, code read MSB-first)
        for s in range(19):
            if cl[s] == length:
                table[(length, code)] = s
                code += 1
        code <<= 1
    lens, used = [], set()
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in table:
            c = (c << 1) | take(1)
            n += 1
            assert n <= 7
        s = table[(n, c)]
        used.add(s)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    assert len(lens) == hlit + hdist
    return btype, lens[:hlit], lens[hlit:], used


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def photo(h):
    rng = np.random.RandomState(0)
    y, x = np.mgrid[0:h, 0:h].astype(np.float64)
    return np.stack([np.clip(127 + 100 * np.sin(x / 17 + c) * np.cos(y / 23) + 6 * rng.randn(h, h), 0, 255) for c in range(3)], -1).astype(np.uint8)


def blocks(h):
    rng = np.random.RandomState(0)
    lab = np.kron(rng.randint(0, 19, (h // 16, h // 16)), np.ones((16, 16), np.int64))
    return ((lab[..., None] * np.array([13, 7, 11])) % 256).astype(np.uint8)


def gradient(h, w, shift=0):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(3 * x + 5 * y + c + shift) % 251 for c in range(3)], -1).astype(np.uint8)


def scrambled_gradient(h, w, shift=0):
    """The gradient through a fixed byte permutation (an affine map of the cube, modulo 251): as many distinct values, but no filter
    leaves three equal bytes in a row, so the chunk holds no match and its block no distance code (asserted where it is used)."""
    g = gradient(h, w, shift).astype(np.int64)
    return ((g * g * g * 5 + 17) % 251).astype(np.uint8)


def outlined_blocks(h):
    img = blocks(h).copy()
    img[10, 10:51] = img[50, 10:51] = (255, 0, 0)
    img[10:51, 10] = img[10:51, 50] = (255, 0, 0)
    return img


def default_rows(w):
    return max(1, min(16, 32768 // (1 + 3 * w)))


def stored_size(h, w, r):
    """Bytes of the stream if every chunk took the stored fallback: header, 5 + bytes per chunk, Adler-32."""
    chunks = -(-h // r)
    return 2 + 5 * chunks + h * (1 + 3 * w) + 4


def _rng_images(h, w, n=2):
    rng = np.random.RandomState(h * 1000 + w)
    return rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)


# name -> (images (n,H,W,3), rows_per_chunk, extra check)
def _cases():
    g = np.stack([gradient(33, 40), gradient(33, 40, 7)])
    cases = {
        "1x1": (np.array([[[[0, 0, 0]]], [[[9, 200, 77]]]], np.uint8), 0, None),
        "1x7": (_rng_images(1, 7), 0, None),
        "7x1": (_rng_images(7, 1), 0, None),
        "23x19-random": (_rng_images(23, 19), 0, "stored"),
        "23x19-zeros": (np.zeros((2, 23, 19, 3), np.uint8), 0, "smaller"),
        "5x100-constant": (np.full((2, 5, 100, 3), 200, np.uint8), 0, "smaller"),
        "33x40-gradient": (g, 0, "smaller"),
        "33x40-no-runs": (np.stack([scrambled_gradient(33, 40), scrambled_gradient(33, 40, 7)]), 0, "no-distance"),
        "33-rows-last-chunk-of-one": (np.stack([gradient(33, 40, 3), photo(64)[:33, :40]]), 16, None),
        "33x40-rows-1": (g, 1, None),
        "33x40-rows-5": (g, 5, None),
        "33x40-rows-H": (g, 33, None),
        "64-photo-blocks": (np.stack([photo(64), outlined_blocks(64)]), 0, None),
        "4x2048": (np.stack([gradient(4, 2048), _rng_images(4, 2048, 1)[0]]), 0, None),
    }
    return cases


CASES = _cases()


def check_streams(name, images, rows, streams, sizes, bound):
    """(i) of the issue for every image of a call.  streams: (n, stride) uint8 whose slots were filled with SENTINEL before the call."""
    n, h, w, _ = images.shape
    r = rows or default_rows(w)
    _, _, extra = CASES.get(name, (None, None, None))
    for i in range(n):
        size = int(sizes[i])
        stream = streams[i, :size].tobytes()
        print("%s[%d]: %d x %d, rows_per_chunk %d: stream %d bytes, stored %d, bound %d" % (name, i, h, w, r, size, stored_size(h, w, r), bound))
        assert size <= bound
        assert (streams[i, size:] == SENTINEL).all(), "bytes behind the stream were written"
        raw = zlib.decompress(stream)                    # (checks the Adler-32)
        assert len(raw) == h * (1 + 3 * w)
        expect = filter_rows(images[i])
        got = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
        assert (got[:, 0] == expect[:, 0]).all(), "filter types differ from the heuristic's"
        assert (got == expect).all()
        assert (unfilter(raw, h, w) == images[i]).all()
        im = Image.open(io.BytesIO(png_container(stream, w, h)))
        im.load()
        assert im.mode == "RGB" and (np.asarray(im) == images[i]).all()
        if extra == "stored":
            assert size == stored_size(h, w, r)
        if extra in ("smaller", "no-distance"):
            assert size < stored_size(h, w, r)
        if extra == "no-distance":
            flat = expect.reshape(-1)
            for c0 in range(0, h, r):                    # no run of three inside a chunk, row boundaries included
                ch = expect[c0:c0 + r].reshape(-1)
                assert not ((ch[2:] == ch[1:-1]) & (ch[1:-1] == ch[:-2])).any()
            btype, lit, dist, used = first_block_header(stream)
            assert btype == 2 and dist == [0], "a block without matches carries no distance code"
            assert flat.size
        if name == "23x19-zeros":
            btype, lit, dist, used = first_block_header(stream)
            assert btype == 2 and dist == [1]
            assert [s for s, l in enumerate(lit) if l][:2] == [0, 256], "one literal value, the end of block, then length symbols only"
            assert 18 in used, "the zero runs of the code lengths use symbol 18"


# ---- CPU: the container, the restatements, the declarations, the simulator ------------------------------------------------------------
def test_container_around_zlib_opens_in_pillow():
    img = photo(64)[:23, :19]
    png = png_container(zlib.compress(filter_rows(img).tobytes()), 19, 23)
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.size == (19, 23) and im.mode == "RGB"
    assert (np.asarray(im) == img).all()


def test_restatements_agree_with_pillow():
    img = photo(64)[:23, :19]
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    raw = zlib.decompress(idat_of(buf.getvalue()))
    mine = filter_rows(img)
    theirs = np.frombuffer(raw, np.uint8).reshape(23, 1 + 3 * 19)
    print("filter types, Pillow:", theirs[:, 0].tolist())
    print("filter types, here:  ", mine[:, 0].tolist())
    assert len(set(theirs[:, 0].tolist())) > 1, "the image should exercise more than one filter type"
    assert (theirs == mine).all()
    assert (unfilter(raw, 23, 19) == img).all()


def test_new_symbols_are_declared():
    header = open(os.path.join(REPO, "include", "swapnet_hip.h")).read()
    for name in ("swn_op_png_encode", "swn_png_stream_bound", "swn_pipeline_enable_png", "swn_pipeline_png"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _C.Lib.exported_symbols()
    assert re.search(r"swn_abi_version.*9|ABI 9", header)


def test_the_host_simulator_refuses_png_by_name():
    ctx = backends.hostsim_ctx()
    with pytest.raises(NotImplementedError, match="simulator"):
        engine.op_png_encode(ctx, torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    assert engine.png_stream_bound(4, 4, 0, lib=ctx.lib) == 2 + (4 * 13 + 5 + 9) + 4        # (plain arithmetic: answered everywhere)
    with pytest.raises(ValueError):
        engine.png_stream_bound(4, 2049, 0, lib=ctx.lib)


# ---- CPU: the encoder's body as host threads ---------------------------------------------------------------------------------------
PNG_HOST_DIR = os.path.join(REPO, "tests", "png_host")
PNG_HOST = os.path.join(PNG_HOST_DIR, "build", "png_host")


def build_png_host():
    deps = [os.path.join(PNG_HOST_DIR, "png_host.cpp"), os.path.join(REPO, "swapnet_amd", "csrc", "png_chunk.h")]
    if os.path.exists(PNG_HOST) and all(os.path.getmtime(d) <= os.path.getmtime(PNG_HOST) for d in deps):
        return PNG_HOST
    os.makedirs(os.path.dirname(PNG_HOST), exist_ok=True)
    tmp = "%s.%d.tmp" % (PNG_HOST, os.getpid())
    try:
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", tmp, deps[0]])
        os.replace(tmp, PNG_HOST)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return PNG_HOST


def host_encode(images, rows, tmp_path):
    n, h, w, _ = images.shape
    src, dst = str(tmp_path / "in.raw"), str(tmp_path / "out.bin")
    np.ascontiguousarray(images).tofile(src)
    subprocess.check_call([build_png_host(), str(h), str(w), str(rows), str(n), src, dst])
    blob = open(dst, "rb").read()
    size0, bound = struct.unpack("<II", blob[:8])
    rec = np.frombuffer(blob, np.uint8).reshape(n, 8 + bound)
    sizes = [struct.unpack("<I", rec[i, :4].tobytes())[0] for i in range(n)]
    return rec[:, 8:], sizes, bound


@pytest.mark.parametrize("name", list(CASES))
def test_host_thread_build_of_the_encoder(name, tmp_path):
    images, rows, _ = CASES[name]
    streams, sizes, bound = host_encode(images, rows, tmp_path)
    check_streams(name, images, rows, streams, sizes, bound)


def pillow_size(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", **kw)
    return len(buf.getvalue())


def host_model_size(img, rows):
    """zlib restricted to run-length matches, one sync-flushed piece per chunk, as a file."""
    f = filter_rows(img)
    total = 2 + 4
    for c0 in range(0, img.shape[0], rows):
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        total += len(z.compress(f[c0:c0 + rows].tobytes()) + z.flush(zlib.Z_SYNC_FLUSH))
    return total + 57


def check_size_caps(streams, sizes):
    p, b = photo(256), blocks(256)
    files = [57 + int(s) for s in sizes]                 # signature 8, IHDR 25, IDAT 12, IEND 12
    pil = [pillow_size(p), pillow_size(b)]
    model = [host_model_size(p, 16), host_model_size(b, 16)]
    print("photo(256):  file %d, Pillow default %d (%.3fx), host RLE model %d" % (files[0], pil[0], files[0] / pil[0], model[0]))
    print("blocks(256): file %d, Pillow default %d (%.3fx), host RLE model %d" % (files[1], pil[1], files[1] / pil[1], model[1]))
    assert files[0] <= pil[0]
    assert files[1] <= 2 * pil[1]


def test_host_thread_build_256_and_the_size_caps(tmp_path):
    images = np.stack([photo(256), blocks(256)])
    streams, sizes, bound = host_encode(images, 0, tmp_path)
    check_streams("256-photo-blocks", images, 0, streams, sizes, bound)
    check_size_caps(streams, sizes)


def test_host_thread_build_refuses_wide_images_and_long_chunks(tmp_path):
    (tmp_path / "in.raw").write_bytes(b"")
    for h, w, r in ((1, 2049, 0), (700, 16, 700)):      # 700 * 49 = 34300 > 32768
        assert subprocess.call([build_png_host(), str(h), str(w), str(r), "1", str(tmp_path / "in.raw"), str(tmp_path / "out.bin")],
                               stderr=subprocess.DEVNULL) == 3


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def device_encode(ctx, images, rows):
    n, h, w, _ = images.shape
    bound = engine.png_stream_bound(h, w, rows)
    out = torch.full((n, bound), SENTINEL, dtype=torch.uint8, device=ctx.device)
    streams, sizes = engine.op_png_encode(ctx, torch.from_numpy(images), rows, out=out)
    assert streams.data_ptr() == out.data_ptr()
    return streams.cpu().numpy(), sizes.cpu().tolist(), bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_streams(name):
    ctx = backends.gpu_ctx()
    images, rows, _ = CASES[name]
    streams, sizes, bound = device_encode(ctx, images, rows)
    check_streams(name, images, rows, streams, sizes, bound)
    again, sizes2, _ = device_encode(ctx, images, rows)                 # (iv) determinism
    assert sizes2 == sizes and (again == streams).all()


@pytest.mark.gpu
def test_device_256_multi_chunk_gather_and_the_size_caps():
    ctx = backends.gpu_ctx()
    images = np.stack([photo(256), blocks(256)])
    streams, sizes, bound = device_encode(ctx, images, 0)
    check_streams("256-photo-blocks", images, 0, streams, sizes, bound)
    check_size_caps(streams, sizes)
    again, sizes2, _ = device_encode(ctx, images, 0)
    assert sizes2 == sizes and (again == streams).all()


@pytest.mark.gpu
def test_device_refuses_wide_images_and_long_chunks():
    ctx = backends.gpu_ctx()
    with pytest.raises(ValueError):
        engine.op_png_encode(ctx, torch.zeros((1, 1, 2049, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        engine.op_png_encode(ctx, torch.zeros((1, 700, 16, 3), dtype=torch.uint8), 700)          # 700 * 49 = 34300 > 32768
    with pytest.raises(ValueError):
        engine.png_stream_bound(700, 16, 700)


@pytest.mark.gpu
def test_encode_png_gives_files_pillow_opens():
    from swapnet_amd.util.png import encode_png
    ctx = backends.gpu_ctx()
    images = np.stack([photo(64), outlined_blocks(64)])
    for src in (images, torch.from_numpy(images), torch.from_numpy(images).to(ctx.device)):
        files = encode_png(ctx, src)
        assert len(files) == 2 and all(isinstance(f, bytes) for f in files)
        for f, img in zip(files, images):
            assert (np.asarray(Image.open(io.BytesIO(f))) == img).all()
