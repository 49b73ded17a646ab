"""Hand-built NV12 / YUYV frames for the YUV sensor tests (test_sensor_yuv_cpu.py, test_gpu_sensor_yuv.py): the planes are written through strided
views of a buffer that is first filled with a padding byte, so every byte a layout does not name keeps that byte."""
import torch

from egotap_amd import spec

COLOURS = [spec.YuvColour(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]


def _views(buf, layout):
    """(Y, U, V) writable views of a uint8 [n, frame_stride] buffer: Y [n, H, W]; U, V [n, H/2, W/2] (nv12) or [n, H, W/2] (yuyv)"""
    n, fs = buf.shape
    H, W, pitch, at = layout.H, layout.W, layout.pitch, buf.storage_offset()
    if layout.format == "nv12":
        return (torch.as_strided(buf, (n, H, W), (fs, pitch, 1), at),
                torch.as_strided(buf, (n, H // 2, W // 2), (fs, pitch, 2), at + layout.uv_offset),
                torch.as_strided(buf, (n, H // 2, W // 2), (fs, pitch, 2), at + layout.uv_offset + 1))
    return (torch.as_strided(buf, (n, H, W), (fs, pitch, 2), at),
            torch.as_strided(buf, (n, H, W // 2), (fs, pitch, 4), at + 1),
            torch.as_strided(buf, (n, H, W // 2), (fs, pitch, 4), at + 3))


def pack(Y, U, V, layout, fill=0):
    """uint8 [n, frame_stride]: the planes Y [n, H, W] and U, V (one value per chroma block) laid out as ``layout`` says, every other byte = fill"""
    buf = torch.full((Y.shape[0], layout.frame_stride), fill, dtype=torch.uint8)
    for view, plane in zip(_views(buf, layout), (Y, U, V)):
        assert tuple(view.shape) == tuple(plane.shape), (view.shape, plane.shape)
        view.copy_(plane)
    return buf


def padding_mask(layout):
    """bool [frame_stride]: True where a byte belongs to no plane"""
    buf = torch.ones((1, layout.frame_stride), dtype=torch.uint8)
    for view in _views(buf, layout):
        view.zero_()
    return buf[0].bool()


def planes(seed, n, layout):
    """random (Y, U, V) planes with 0 and 255 in every plane of every frame"""
    g = torch.Generator().manual_seed(seed)
    H, W = layout.H, layout.W
    ch = (H // 2, W // 2) if layout.format == "nv12" else (H, W // 2)
    out = [torch.randint(0, 256, (n,) + s, generator=g, dtype=torch.uint8) for s in ((H, W), ch, ch)]
    for p in out:
        p[:, 0, 0] = 0
        p[:, -1, -1] = 255
    return out


def frames(seed, n, layout, fill=0):
    return pack(*planes(seed, n, layout), layout, fill)


def rgb_by_hand(Y, U, V, layout, colour):
    """uint8 [n, H, W, 3] from the planes, with the chroma of pixel (y, x) picked by index arithmetic ((y >> 1, x >> 1) for nv12, (y, x >> 1) for yuyv)"""
    H, W = layout.H, layout.W
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    cy = (ys >> 1) if layout.format == "nv12" else ys
    u, v = U[:, cy, xs >> 1], V[:, cy, xs >> 1]
    return torch.stack(spec.yuv_rgb_bytes(Y, u, v, colour), dim=-1).to(torch.uint8)


def all_triples_nv12():
    """(frame uint8 [1, frame_stride], layout): a tight 4096 x 4096 NV12 frame whose 2 x 2 blocks enumerate every (Y, U, V): block k (row-major over
    2048 x 2048) holds U = k >> 14, V = (k >> 6) & 255 and the four Y values 4 (k & 63) .. 4 (k & 63) + 3"""
    layout = spec.YuvLayout.nv12(4096, 4096)
    k = torch.arange(2048 * 2048, dtype=torch.int64).view(2048, 2048)
    U, V = (k >> 14).to(torch.uint8), ((k >> 6) & 255).to(torch.uint8)
    y4 = 4 * (k & 63)
    Y = torch.empty((4096, 4096), dtype=torch.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            Y[dy::2, dx::2] = (y4 + 2 * dy + dx).to(torch.uint8)
    return pack(Y[None], U[None], V[None], layout), layout


def lattice_nv12(values=(0, 16, 128, 235, 240, 255)):
    """(frame, layout): a tight 512 x 512 NV12 frame over a 64-value lattice that holds ``values``: block k holds U = lat[k >> 10], V = lat[(k >> 4) & 63]
    and the Y values lat[4 (k & 15) .. + 3]"""
    rest = [v for v in range(1, 255, 4) if v not in values]
    lat = torch.tensor(sorted(list(values) + rest[:64 - len(values)]), dtype=torch.uint8)
    assert lat.numel() == 64 and len(set(lat.tolist())) == 64
    layout = spec.YuvLayout.nv12(512, 512)
    k = torch.arange(256 * 256, dtype=torch.int64).view(256, 256)
    U, V = lat[k >> 10], lat[(k >> 4) & 63]
    Y = torch.empty((512, 512), dtype=torch.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            Y[dy::2, dx::2] = lat[4 * (k & 15) + 2 * dy + dx]
    return pack(Y[None], U[None], V[None], layout), layout
