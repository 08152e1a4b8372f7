"""CPU: the Radiance .hdr readers (vpt_amd/hdr.py, js/vpt/hdr.js) against the small RGBE encoder below — new-style run-length and flat
scanlines, widths on both sides of the run-length limits, runs around the 127-byte record limit, both magic lines, extra header lines — and
what they refuse.  Python's and Node's readers return the same bytes.  The hosts' dispatch of environment maps refuses what is no map before
any device call."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from vpt_amd.hdr import HDRImage, read_hdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


def rle_channel(v, min_run=3):
    """one channel plane of a new-style scanline: runs of >= min_run equal bytes as (128 + n, byte) records of at most 127, the rest as
    literal records of at most 128 bytes"""
    out, i, n = bytearray(), 0, len(v)
    while i < n:
        j = i
        while j < n and v[j] == v[i] and j - i < 127:
            j += 1
        if j - i >= min_run:
            out += bytes([128 + j - i, v[i]]); i = j
            continue
        k = i
        while k < n and k - i < 128 and not (k + min_run <= n and min_run > 1 and all(v[k + t] == v[k] for t in range(min_run))):
            k += 1
        k = max(k, i + 1)
        out += bytes([k - i]) + bytes(v[i:k]); i = k
    return bytes(out)


def encode_hdr(rgbe, rle=True, magic=b"#?RADIANCE", extra=(), fmt=b"32-bit_rle_rgbe", resolution=None, min_run=3):
    h, w, _ = rgbe.shape
    out = [magic + b"\n"] + [line + b"\n" for line in extra]
    if fmt is not None:
        out.append(b"FORMAT=" + fmt + b"\n")
    out.append(b"\n" + (resolution or b"-Y %d +X %d" % (h, w)) + b"\n")
    for row in rgbe:
        if rle and 8 <= w <= 32767:
            out.append(bytes([2, 2, w >> 8, w & 255]))
            for c in range(4):
                out.append(rle_channel(row[:, c].tobytes(), min_run))
        else:
            out.append(row.tobytes())
    return b"".join(out)


def rgbe_image(h, w, seed=0):
    """random RGBE bytes with stretches of equal bytes; no (1, 1, 1, n) pixel (a flat scanline would read it as an old-style run)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    for _ in range(max(1, w // 16)):
        y, x, c = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, 4))
        img[y, x:x + int(rng.integers(1, 40)), c] = img[y, x, c]
    img[(img[..., 0] == 1) & (img[..., 1] == 1) & (img[..., 2] == 1), 0] = 7
    return img


@pytest.mark.parametrize("rle", [True, False])
@pytest.mark.parametrize("w", [1, 7, 8, 300, 32768])
def test_round_trip_widths(w, rle):
    img = rgbe_image(3 if w < 32768 else 2, w, seed=w)
    got = read_hdr(encode_hdr(img, rle=rle))
    assert isinstance(got, HDRImage) and got.format == 'rgbe'
    assert (got.width, got.height) == (w, img.shape[0])
    assert got.data.dtype == np.uint8 and got.data.shape == img.shape
    assert got.data.tobytes() == img.tobytes()


@pytest.mark.parametrize("run", [1, 127, 128, 129, 255])
@pytest.mark.parametrize("min_run", [1, 3])
def test_round_trip_runs(run, min_run):
    """a stretch of `run` equal bytes in each channel (min_run = 1: every byte in a run record, 129 for a single byte)"""
    w = 300
    img = rgbe_image(2, w, seed=run)
    for c in range(4):
        img[:, 10 + c:10 + c + run, c] = 200 + c
    data = encode_hdr(img, min_run=min_run)
    if min_run == 1:
        assert data.count(bytes([129])) > 0
    assert read_hdr(data).data.tobytes() == img.tobytes()


def test_literal_records_of_128_bytes():
    img = np.arange(2 * 300 * 4, dtype=np.uint32).astype(np.uint8).reshape(2, 300, 4)
    img[..., 0] = np.arange(300) % 251                                 # (no two neighbours equal: literal records only)
    data = encode_hdr(img)
    assert bytes([128]) in data
    assert read_hdr(data).data.tobytes() == img.tobytes()


@pytest.mark.parametrize("magic", [b"#?RADIANCE", b"#?RGBE"])
@pytest.mark.parametrize("extra,fmt", [((), b"32-bit_rle_rgbe"), ((), None),
                                       ((b"# made by a test", b"EXPOSURE=2.5", b"PRIMARIES=0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329",
                                         b"SOFTWARE=x"), b"32-bit_rle_rgbe")])
def test_header_forms(tmp_path, magic, extra, fmt):
    """EXPOSURE is read past, not applied: the bytes are the file's"""
    img = rgbe_image(4, 16, seed=1)
    data = encode_hdr(img, magic=magic, extra=extra, fmt=fmt)
    assert read_hdr(data).data.tobytes() == img.tobytes()
    p = tmp_path / "map.hdr"
    p.write_bytes(data)
    assert read_hdr(str(p)).data.tobytes() == img.tobytes()            # a path reads the same
    assert read_hdr(p).data.tobytes() == img.tobytes()


def bad_files():
    img = rgbe_image(3, 16, seed=2)
    good = encode_hdr(img)
    old = img.copy(); old[1, 0, :3] = 1; old[1, 0, 3] = 4              # (1, 1, 1, n): an old-style repeat
    wrong_width = bytearray(good)
    at = good.index(b"\n-Y 3 +X 16\n") + len(b"\n-Y 3 +X 16\n")
    wrong_width[at + 3] = 15
    zero = bytearray(good); zero[at + 4] = 0
    return {
        "xyze": encode_hdr(img, fmt=b"32-bit_rle_xyze"),
        "+Y": encode_hdr(img, resolution=b"+Y 3 +X 16"),
        "-X": encode_hdr(img, resolution=b"-Y 3 -X 16"),
        "+X first": encode_hdr(img, resolution=b"+X 16 -Y 3"),
        "old-style": encode_hdr(old, rle=False),
        "old-style narrow": encode_hdr(np.ones((1, 4, 4), np.uint8), rle=False),
        "truncated": good[:-5],
        "truncated flat": encode_hdr(img, rle=False)[:-1],
        "truncated header": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n",
        "scanline width": bytes(wrong_width),
        "zero count": bytes(zero),
        "magic": b"#?RADIANCEX\n\n-Y 1 +X 1\n\x01\x02\x03\x80",
        "empty": encode_hdr(img[:0], resolution=b"-Y 0 +X 16"),
    }


@pytest.mark.parametrize("name", sorted(bad_files()))
def test_refused(name):
    with pytest.raises(ValueError, match="HDR: "):
        read_hdr(bad_files()[name])


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_reader_returns_the_same_bytes(tmp_path):
    files = {"w%d_%s" % (w, rle): encode_hdr(rgbe_image(3 if w < 32768 else 2, w, seed=w), rle=rle)
             for w in (1, 7, 8, 300, 32768) for rle in (True, False)}
    img = rgbe_image(2, 300, seed=9)
    img[:, 3:258, 1] = 77
    files["runs"] = encode_hdr(img, min_run=1)
    files["header"] = encode_hdr(rgbe_image(4, 16, seed=1), magic=b"#?RGBE", extra=(b"EXPOSURE=2.5", b"# c"), fmt=None)
    files.update({"bad " + k: v for k, v in bad_files().items()})
    names = sorted(files)
    for i, k in enumerate(names):
        (tmp_path / ("%d.hdr" % i)).write_bytes(files[k])
    script = ("const fs = require('fs'); const { readHDR } = require(%s); const out = [];"
              "for (const p of process.argv.slice(1)) { try { const r = readHDR(fs.readFileSync(p)); fs.writeFileSync(p + '.rgbe', r.data);"
              " out.push({ width: r.width, height: r.height, format: r.format }); } catch (e) { out.push({ error: e.message }); } }"
              "console.log(JSON.stringify(out));") % json.dumps(os.path.join(ROOT, "js", "vpt", "hdr.js"))
    res = subprocess.run([NODE, "-e", script] + [str(tmp_path / ("%d.hdr" % i)) for i in range(len(names))],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert res.returncode == 0, res.stdout.decode()
    got = json.loads(res.stdout.decode())
    for i, k in enumerate(names):
        if k.startswith("bad "):
            assert "error" in got[i] and got[i]["error"].startswith("HDR: "), (k, got[i])
            continue
        want = read_hdr(files[k])
        assert got[i] == {"width": want.width, "height": want.height, "format": "rgbe"}, k
        assert (tmp_path / ("%d.hdr.rgbe" % i)).read_bytes() == want.data.tobytes(), k


def test_python_host_refuses_what_is_no_environment_map():
    """checked before any device call (the renderer below has no native handle)"""
    from vpt_amd.renderers import MCMRenderer
    r = MCMRenderer.__new__(MCMRenderer)
    r._h = None
    for bad, err in [([[[255, 255, 255, 255]]], TypeError), (np.zeros((2, 2, 4), np.int32), TypeError), (np.zeros((2, 2, 4), np.float64), TypeError),
                     (np.zeros((2, 2, 3), np.uint8), ValueError), (np.zeros((2, 2, 2), np.float32), ValueError),
                     (np.zeros((2, 8), np.float32), ValueError), ("map.hdr", TypeError),
                     (HDRImage(np.zeros((2, 3, 4), np.uint8), 2, 2), ValueError)]:
        with pytest.raises(err):
            r._upload_environment(bad)


def test_abi_refuses_null_arguments_without_a_gpu():
    import ctypes as C
    from vpt_amd import _native as N
    L = N.lib()
    texel = (C.c_float * 4)(1, 1, 1, 1)
    assert L.vpt_renderer_set_environment_texels(None, texel, 1, 1, N.ENV_RGBA32F) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    assert L.vpt_probe_environment_texels(None, texel, 1) == N.ERR_INVALID
