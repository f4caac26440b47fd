"""``write_mesh_obj``, ``write_png`` and ``read_png``: an OBJ with its MTL and its atlas as a PNG, read back.
CPU only."""
import os
import zlib

import numpy as np
import pytest

import component_scene as cs
import texture_oracle as to
import texture_scene as ts


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.mark.parametrize("channels", (1, 3))
def test_obj_mtl_png_round_trip(pkg, tmp_path, channels):
    m = cs.oracle_mesh("sphere", 1)
    r = to.texture(m, 3, channels, ts.views())
    nt = len(m["faces"])
    atlas = pkg.TextureAtlas(r["atlas"][:, :, 0] if channels == 1 else r["atlas"], r["uv"], r["view"], r["score"], r["n_textured"])
    path = str(tmp_path / "sphere.obj")
    pkg.write_mesh_obj(path, m["vertices"], m["faces"], atlas)
    assert sorted(os.listdir(tmp_path)) == ["sphere.mtl", "sphere.obj", "sphere.png"]
    # the PNG: decoded by read_png to the atlas bit for bit (B, G, R order again), and every row carries filter 0
    back = pkg.read_png(str(tmp_path / "sphere.png"))
    assert back.dtype == np.uint8 and np.array_equal(back, atlas.atlas)
    raw = open(tmp_path / "sphere.png", "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[24] == 8 and raw[25] == (0 if channels == 1 else 2)
    side = atlas.atlas.shape[0]
    at = raw.index(b"IDAT")
    n = int.from_bytes(raw[at - 4:at], "big")
    rows = np.frombuffer(zlib.decompress(raw[at + 4:at + 4 + n]), np.uint8).reshape(side, 1 + side * channels)
    assert (rows[:, 0] == 0).all()
    if channels == 3:                                        # R, G, B in the file
        assert np.array_equal(rows[:, 1:].reshape(side, side, 3), atlas.atlas[:, :, ::-1])
    # the OBJ: v, then 3 vt a triangle with 1 - v, then faces of v/vt
    lines = open(path).read().splitlines()
    assert lines[0] == "mtllib sphere.mtl" and lines[1] == "usemtl sphere"
    v = [ln.split()[1:] for ln in lines if ln.startswith("v ")]
    vt = [ln.split()[1:] for ln in lines if ln.startswith("vt ")]
    f = [ln.split()[1:] for ln in lines if ln.startswith("f ")]
    assert len(v) == len(m["vertices"]) and len(vt) == 3 * nt and len(f) == nt
    assert np.array_equal(np.array(v, np.float64), m["vertices"])                               # %.17g: bit for bit
    uv = np.array(vt, np.float64).reshape(nt, 3, 2)
    assert np.array_equal(uv[:, :, 0], r["uv"][:, :, 0]) and np.array_equal(uv[:, :, 1], 1.0 - r["uv"][:, :, 1])
    corners = np.array([[[int(x) for x in c.split("/")] for c in face] for face in f])
    assert all(c.count("/") == 1 for face in f for c in face)
    assert np.array_equal(corners[:, :, 0] - 1, m["faces"]) and np.array_equal(corners[:, :, 1] - 1, np.arange(3 * nt).reshape(nt, 3))
    mtl = open(tmp_path / "sphere.mtl").read()
    assert mtl.startswith("newmtl sphere\n") and "map_Kd sphere.png" in mtl


def test_read_png_undoes_every_row_filter(pkg, tmp_path):
    """A PNG whose rows use the filters 0 to 4, made by hand: read_png gives the image back."""
    import struct
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (5, 6, 3), dtype=np.uint8)
    flat = img[:, :, ::-1].reshape(5, -1).astype(np.int64)
    rows = []
    for y in range(5):
        up = flat[y - 1] if y else np.zeros(18, np.int64)
        left = np.concatenate([np.zeros(3, np.int64), flat[y][:-3]])
        ul = np.concatenate([np.zeros(3, np.int64), up[:-3]])
        pa, pb, pc = abs(up - ul), abs(left - ul), abs(left + up - 2 * ul)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        pred = (np.zeros(18, np.int64), left, up, (left + up) >> 1, paeth)[y]
        rows.append(bytes([y]) + ((flat[y] - pred) & 255).astype(np.uint8).tobytes())
    chunk = lambda k, d: struct.pack(">I", len(d)) + k + d + struct.pack(">I", zlib.crc32(k + d) & 0xFFFFFFFF)
    path = str(tmp_path / "f.png")
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 5, 8, 2, 0, 0, 0)) +
                 chunk(b"IDAT", zlib.compress(b"".join(rows))) + chunk(b"IEND", b""))
    assert np.array_equal(pkg.read_png(path), img)
    with pytest.raises(ValueError):
        pkg.write_mesh_obj(str(tmp_path / "x.obj"), np.zeros((3, 3)), np.zeros((2, 3), np.int64),
                           pkg.TextureAtlas(np.zeros((4, 4), np.uint8), np.zeros((1, 3, 2)), np.zeros(1, np.int32), np.zeros(1), 0))
