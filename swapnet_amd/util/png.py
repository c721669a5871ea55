"""PNG files from the device's zlib streams: what util.save_image (util/util.py:54-69, Image.fromarray(a).save(path)) leaves on disk,
with the filtering and the deflate done by engine.op_png_encode (csrc/png_encode.hip) and only the container assembled here."""
import struct
import zlib

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_container(zlib_stream, width, height):
    """Signature, IHDR (8-bit, colour type 2 = RGB, no interlace), ONE IDAT holding `zlib_stream` (the zlib stream of the filtered
    scanlines), IEND."""
    ihdr = struct.pack(">IIBBBBB", int(width), int(height), 8, 2, 0, 0, 0)
    return PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", bytes(zlib_stream)) + _chunk(b"IEND", b"")


def encode_png(ctx, images_u8, rows_per_chunk=0):
    """(n,H,W,3) uint8, device or host (torch tensor or numpy array) -> list of n PNG files as bytes.  Two device-to-host copies:
    the n sizes, then the used part of the streams."""
    from .. import engine
    streams, sizes = engine.op_png_encode(ctx, images_u8, rows_per_chunk)
    n, h, w = int(images_u8.shape[0]), int(images_u8.shape[1]), int(images_u8.shape[2])
    sz = sizes.cpu().tolist()
    used = streams[:, :max(sz)].cpu().numpy()
    return [png_container(used[i, :sz[i]].tobytes(), w, h) for i in range(n)]


def save_png(path, png_bytes):
    with open(path, "wb") as f:
        f.write(png_bytes)
