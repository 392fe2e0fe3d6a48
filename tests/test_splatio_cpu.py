"""No GPU: the viewer formats of mojosplat_amd/splatio.py with backend="torch", the definition.  The compressed PLY and the
.splat row are pinned bit for bit against a SCALAR restatement of both formats held in this file (one Gaussian at a time,
numpy.float32 arithmetic and Python ints, no code shared with the module); the round-trip error stays inside bounds derived
from the bit widths; files, headers, every ValueError, foreign 12-float chunks; the argument checks of the four C entries."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _hip, splatio
from mojosplat_amd.knn import SH_C0
from mojosplat_amd.scene_order import morton_permutation
from splatio_cases import (HAND_K, HAND_N, KEYS, KS, NS, ROW_EQUAL_ALL, ROW_EQUAL_PAIR, ROW_NEGATIVE_LARGEST, ROW_OPACITY_0,
                           ROW_OPACITY_1, ROW_SCALE_HIGH, ROW_SCALE_LOW, ROW_SH, hand_built_scene, seeded_scene)

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# the scalar restatement.  The prepared inputs are the documented torch conversions (they are not part of the exact format);
# everything after them is numpy.float32 scalars and Python ints.

def prepared(p, space):
    q, s, o, f = p["quats"], p["scales"], p["opacities"], p["features"]
    N, K = f.shape[0], f.shape[1]
    rot = q / q.norm(dim=1, keepdim=True)
    lsc = s.clamp(-20, 20)
    alpha = torch.sigmoid(o) if space == "logit" else o
    rgba = torch.cat([f[:, 0, :] * SH_C0 + 0.5, alpha[:, None]], 1)
    shr = f[:, 1:, :].transpose(1, 2).reshape(N, 3 * (K - 1))
    return [x.contiguous().numpy().astype(F) for x in (p["means3d"], rot, lsc, rgba, shr)] + [torch.exp(s).numpy().astype(F)]


def s_norm(v, lo, hi):
    if v <= lo:
        return F(0)
    if v >= hi:
        return F(1)
    if F(hi - lo) < F(1e-5):
        return F(0)
    return F(F(v - lo) / F(hi - lo))


def s_pack(v, b):
    t = F((1 << b) - 1)
    return int(min(t, max(F(0), np.floor(F(F(v * t) + F(0.5))))))


def s_byte(x):
    return int(min(F(255), max(F(0), np.trunc(x))))


def s_rotation(a):
    a = [F(x) for x in a]
    L = 0
    for i in range(1, 4):
        if abs(a[i]) > abs(a[L]):
            L = i
    if a[L] < 0:
        a = [F(-x) for x in a]
    word = L
    for i in range(4):
        if i != L:
            word = word << 10 | s_pack(F(F(a[i] * F(0.70710678)) + F(0.5)), 10)
    return word


def spec_compress(pos, rot, lsc, rgba, shr):
    """-> chunks (C, 18) float32, words (N, 4) as Python ints, sh bytes (N, R)."""
    N = pos.shape[0]
    C = -(-N // 256)
    chunks = np.zeros((C, 18), F)
    words = []
    for c in range(C):
        rows = range(256 * c, min(256 * c + 256, N))
        for base, src in ((0, pos), (6, lsc), (12, rgba)):
            for k in range(3):
                chunks[c, base + k] = min(src[i, k] for i in rows)
                chunks[c, base + 3 + k] = max(src[i, k] for i in rows)
        ch = chunks[c]
        for i in rows:
            n = [s_norm(pos[i, k], ch[k], ch[3 + k]) for k in range(3)]
            position = s_pack(n[0], 11) << 21 | s_pack(n[1], 10) << 11 | s_pack(n[2], 11)
            n = [s_norm(lsc[i, k], ch[6 + k], ch[9 + k]) for k in range(3)]
            scale = s_pack(n[0], 11) << 21 | s_pack(n[1], 10) << 11 | s_pack(n[2], 11)
            n = [s_norm(rgba[i, k], ch[12 + k], ch[15 + k]) for k in range(3)]
            colour = s_pack(n[0], 8) << 24 | s_pack(n[1], 8) << 16 | s_pack(n[2], 8) << 8 | s_pack(rgba[i, 3], 8)
            words.append([position, s_rotation(rot[i]), scale, colour])
    sh = [[s_byte(F(F(F(v / F(8)) + F(0.5)) * F(256))) for v in row] for row in shr]
    return chunks, words, sh


def s_unit(x, b):
    m = (1 << b) - 1
    return F(F(x & m) / F(m))


def s_mix(lo, hi, u):
    return F(F(lo * F(F(1) - u)) + F(hi * u))


def spec_decompress_row(ch, w, sh_row):
    """A chunk row of 18 floats, four words and the SH bytes -> pos, rot, lsc, rgba, shr as lists of float32."""
    p, r, s, c = w
    pos = [s_mix(ch[0], ch[3], s_unit(p >> 21, 11)), s_mix(ch[1], ch[4], s_unit(p >> 11, 10)), s_mix(ch[2], ch[5], s_unit(p, 11))]
    lsc = [s_mix(ch[6], ch[9], s_unit(s >> 21, 11)), s_mix(ch[7], ch[10], s_unit(s >> 11, 10)), s_mix(ch[8], ch[11], s_unit(s, 11))]
    rgba = [s_mix(ch[12], ch[15], s_unit(c >> 24, 8)), s_mix(ch[13], ch[16], s_unit(c >> 16, 8)),
            s_mix(ch[14], ch[17], s_unit(c >> 8, 8)), s_unit(c, 8)]
    L = r >> 30
    a, b, d = (F(F(s_unit(r >> k, 10) - F(0.5)) * F(1.41421356)) for k in (20, 10, 0))
    m = np.sqrt(max(F(0), F(F(F(F(1) - F(a * a)) - F(b * b)) - F(d * d))))
    rot = [a, b, d]
    rot.insert(L, F(m))
    shr = [F(F(F(x) * F(F(8.0) / F(255.0))) - F(4.0)) for x in sh_row]
    return pos, rot, lsc, rgba, shr


def spec_splat_rows(pos, scale_lin, rgba, rot):
    out = []
    for i in range(pos.shape[0]):
        row = pos[i].astype("<f4").tobytes() + scale_lin[i].astype("<f4").tobytes()
        row += bytes(s_byte(F(v * F(255))) for v in rgba[i])
        row += bytes(s_byte(F(F(r * F(128)) + F(128))) for r in rot[i])
        out.append(row)
    return b"".join(out)


def as_uint(vertices):
    return [[int(x) & 0xFFFFFFFF for x in row] for row in vertices.tolist()]


def check_against_spec(p, space):
    pos, rot, lsc, rgba, shr, scale_lin = prepared(p, space)
    K = p["features"].shape[1]
    cs = ms.compress_scene(p, opacity_space=space, order="keep", backend="torch")
    chunks, words, sh = spec_compress(pos, rot, lsc, rgba, shr)
    assert cs.K == K and cs.chunks.dtype == torch.float32 and cs.vertices.dtype == torch.int32
    assert np.array_equal(cs.chunks.numpy().view(np.int32), chunks.view(np.int32))
    assert as_uint(cs.vertices) == words
    assert torch.equal(cs.perm, torch.arange(pos.shape[0]))
    if K == 1:
        assert cs.sh is None
    else:
        assert cs.sh.dtype == torch.uint8 and cs.sh.tolist() == sh
    # ... and the decoder, on what the encoder produced
    dec = [x.numpy() if x is not None else None for x in splatio._decompress_torch(cs.chunks, cs.vertices, cs.sh)]
    for i in range(0, pos.shape[0], 7):
        want = spec_decompress_row(chunks[i // 256], words[i], sh[i] if K > 1 else [])
        for got, w in zip(dec, want):
            if got is not None:
                assert np.array_equal(got[i].view(np.int32), np.array(w, F).view(np.int32)), i
    rows, perm = splatio.pack_splat_rows(p, opacity_space=space, order="keep", backend="torch")
    assert rows.dtype == torch.uint8 and rows.shape == (pos.shape[0], 32) and torch.equal(perm, torch.arange(pos.shape[0]))
    assert rows.numpy().tobytes() == spec_splat_rows(pos, scale_lin, rgba, rot)
    return cs, rows


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_the_definition_equals_the_scalar_restatement(N, K):
    with np.errstate(all="ignore"):
        check_against_spec(seeded_scene(N, K), "logit")


def test_the_hand_built_cases_equal_the_scalar_restatement():
    p = hand_built_scene()
    with np.errstate(all="ignore"):
        cs, rows = check_against_spec(p, "linear")
    w = as_uint(cs.vertices)
    assert all(w[i][0] == 0 for i in range(256, HAND_N)) and any(w[i][0] for i in range(256))        # one position: word 0
    assert torch.equal(cs.chunks[1, 0:3], cs.chunks[1, 3:6])
    # the largest component negative: index 1, and the others' signs flipped (w = 0.1 -> -0.1 -> below the middle code 512)
    assert w[ROW_NEGATIVE_LARGEST][1] >> 30 == 1 and (w[ROW_NEGATIVE_LARGEST][1] >> 20 & 1023) < 512
    assert w[ROW_EQUAL_PAIR][1] >> 30 == 1 and (w[ROW_EQUAL_PAIR][1] >> 10 & 1023) < 512              # x = 0.7 wins, y = -0.7 stays negative
    assert w[ROW_EQUAL_ALL][1] >> 30 == 0 and all((w[ROW_EQUAL_ALL][1] >> s & 1023) < 512 for s in (20, 10, 0))
    assert float(cs.chunks[0, 6]) == -20.0 and float(cs.chunks[0, 10]) == 20.0                         # the clamp
    assert w[ROW_SCALE_LOW][2] >> 21 == 0 and w[ROW_SCALE_HIGH][2] >> 11 & 1023 == 1023
    assert cs.sh[ROW_SH, 0::HAND_K - 1].tolist() == [0, 255, 255]                                      # -5, 4, 3.99: k = 1 of each channel
    assert w[ROW_OPACITY_0][3] & 255 == 0 and w[ROW_OPACITY_1][3] & 255 == 255
    assert rows[ROW_OPACITY_0, 27] == 0 and rows[ROW_OPACITY_1, 27] == 255
    d = ms.decompress_scene(cs, backend="torch")                                                      # bytes 0 and 255 stay finite
    assert bool(torch.isfinite(d["opacities"]).all())
    assert float(d["opacities"][ROW_OPACITY_0]) == pytest.approx(math.log(1 / 509), rel=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# round-trip error: bounds from the bit widths

SLACK = 1.0 + 1e-3


def test_round_trip_error_is_inside_the_bit_widths():
    """N = 700, K = 16, file order = scene order: chunks of 256, 256 and 188 random rows, so every chunk's range is several
    units wide against values below 5 -- the float32 arithmetic of the decoder (four roundings of at most 2^-24 relative on
    values of that size, about 1e-6) fits the 1e-3 relative slack on bounds that are 1e-3 of the range or more."""
    p = seeded_scene(700, 16, seed=3)
    pos, rot, lsc, rgba, shr, _ = prepared(p, "logit")
    cs = ms.compress_scene(p, order="keep", backend="torch")
    dpos, drot, dlsc, drgba, dshr = (x.numpy() for x in splatio._decompress_torch(cs.chunks, cs.vertices, cs.sh))
    per = np.repeat(cs.chunks.numpy(), 256, 0)[:700].astype(np.float64)
    for got, want, base in ((dpos, pos, 0), (dlsc, lsc, 6)):
        rng = per[:, base + 3:base + 6] - per[:, base:base + 3]
        err = np.abs(got.astype(np.float64) - want)
        # x and z have 11 bits: 2047 steps over the range, rounded to the nearest code, so half a step; y has 10 bits: 1023
        assert (err[:, 0] <= rng[:, 0] / (2 * 2047) * SLACK).all() and (err[:, 2] <= rng[:, 2] / (2 * 2047) * SLACK).all()
        assert (err[:, 1] <= rng[:, 1] / (2 * 1023) * SLACK).all()
        assert err.max() > 0
    # colour: 8 bits, 255 steps over the chunk's range, half a step
    rng = per[:, 15:18] - per[:, 12:15]
    assert (np.abs(drgba[:, :3].astype(np.float64) - rgba[:, :3]) <= rng / 510 * SLACK).all()
    # opacity: 255 steps over [0, 1], half a step
    assert (np.abs(drgba[:, 3].astype(np.float64) - rgba[:, 3]) <= 1 / 510 * SLACK).all()
    # rotation: a component c is stored as c / sqrt(2) + 0.5 on 1023 steps (half a step: 1 / 2046) and read back times sqrt(2)
    a = rot.astype(np.float64)
    L = np.abs(rot).argmax(1)
    a = a * np.where(a[np.arange(700), L] < 0, -1.0, 1.0)[:, None]
    keep = np.ones((700, 4), bool)
    keep[np.arange(700), L] = False
    assert (np.abs(drot.astype(np.float64) - a)[keep] <= math.sqrt(2) / (2 * 1023) * SLACK).all()
    # ... and the whole quaternion: component errors <= 7e-4 each; the rebuilt one, m = sqrt(1 - the others' squares) >= 0.5 (the
    # largest of four), is off by at most sum |c| dc / m <= 3 * 0.71 * 7e-4 / 0.5 = 3e-3; |q . q0| = 1 - |dq|^2 / 2 >= 1 - 1e-4
    assert ((drot.astype(np.float64) * a).sum(1) >= 1 - 1e-4).all()
    # SH: the byte is floor((v / 8 + 0.5) * 256), up to a step of 8 / 256 below v; it is read back on 255 steps, byte * 8 / 255 - 4,
    # which moves byte b by b * 8 * (1 / 255 - 1 / 256) <= 8 / 255 more
    inside = np.abs(shr) < 4
    assert inside.mean() > 0.9 and not inside.all()
    assert (np.abs(dshr.astype(np.float64) - shr)[inside] <= (8 / 255 + 8 / 256) * SLACK).all()


# ---------------------------------------------------------------------------------------------------------------------------
# files

def _same(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in KEYS)


def expected_header(N, K):
    lines = ["ply", "format binary_little_endian 1.0", f"element chunk {-(-N // 256)}"]
    lines += ["property float " + n for n in
              "min_x min_y min_z max_x max_y max_z min_scale_x min_scale_y min_scale_z max_scale_x max_scale_y max_scale_z "
              "min_r min_g min_b max_r max_g max_b".split()]
    lines += [f"element vertex {N}"] + ["property uint packed_" + n for n in ("position", "rotation", "scale", "color")]
    if K > 1:
        lines += [f"element sh {N}"] + [f"property uchar f_rest_{i}" for i in range(3 * (K - 1))]
    return ("\n".join(lines + ["end_header"]) + "\n").encode()


@pytest.mark.parametrize("K", (1, 9))
def test_a_saved_file_is_the_header_and_the_three_elements_and_loads_back(tmp_path, K):
    N = 300
    p = seeded_scene(N, K, seed=5)
    before = {k: v.clone() for k, v in p.items()}
    path = str(tmp_path / "scene.compressed.ply")
    n = ms.save_compressed_ply(path, p, backend="torch")
    assert _same(p, before) and not os.path.exists(path + ".tmp")
    data = open(path, "rb").read()
    cs = ms.compress_scene(p, backend="torch")
    head = expected_header(N, K)
    body = cs.chunks.numpy().tobytes() + cs.vertices.numpy().tobytes() + (cs.sh.numpy().tobytes() if K > 1 else b"")
    assert n == len(data) == len(head) + 72 * 2 + 16 * N + 3 * (K - 1) * N and data == head + body
    assert sorted(cs.perm.tolist()) == list(range(N)) and torch.equal(cs.perm, morton_permutation(p["means3d"]))
    got = ms.load_compressed_ply(path, backend="torch", requires_grad=True)
    want = ms.decompress_scene(cs, backend="torch")
    assert _same(got, want) and got["features"].shape == (N, K, 3) and got["opacities"].shape == (N,)
    assert all(v.is_leaf and v.requires_grad and v.is_contiguous() and v.dtype == torch.float32 and v.device.type == "cpu"
               for v in got.values())
    lin = ms.load_compressed_ply(path, backend="torch", opacity_space="linear")
    assert torch.equal(lin["opacities"], (cs.vertices[:, 3] & 255).float() / 255)
    # the file is close to the scene it came from, in file order
    assert float((got["means3d"].detach() - p["means3d"][cs.perm]).abs().max()) < 0.01


def test_rgb_features_and_linear_opacities_go_through_the_same_conversions():
    g = torch.Generator().manual_seed(2)
    N = 40
    p = seeded_scene(N, 1, seed=9)
    rgb = {**p, "features": torch.rand((N, 3), generator=g), "opacities": torch.rand((N,), generator=g)}
    sh = {**rgb, "features": ((rgb["features"] - 0.5) / SH_C0).unsqueeze(1)}
    a, b = (ms.compress_scene(x, opacity_space="linear", order="keep", backend="torch") for x in (rgb, sh))
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.chunks, b.chunks) and a.K == 1 and a.sh is None


def test_splat_files(tmp_path):
    p = seeded_scene(2, 4, seed=1)
    path = str(tmp_path / "two.splat")
    assert ms.save_splat(path, p, backend="torch") == 64 and os.path.getsize(path) == 64 and not os.path.exists(path + ".tmp")
    p = seeded_scene(300, 4, seed=1)
    rows, perm = splatio.pack_splat_rows(p, backend="torch")
    lin = torch.sigmoid(p["opacities"])
    key = -(torch.exp((p["scales"][:, 0] + p["scales"][:, 1]) + p["scales"][:, 2]) * lin)
    assert torch.equal(perm, torch.argsort(key, stable=True)) and bool((key[perm][1:] >= key[perm][:-1]).all())
    keep, ident = splatio.pack_splat_rows(p, order="keep", backend="torch")
    assert torch.equal(rows, keep[perm]) and torch.equal(ident, torch.arange(300))
    assert ms.save_splat(path, p, backend="torch") == 9600 and open(path, "rb").read() == rows.numpy().tobytes()
    got = ms.load_splat(path, backend="torch")
    assert got["features"].shape == (300, 1, 3) and all(v.is_leaf and v.is_contiguous() and v.dtype == torch.float32 for v in got.values())
    assert _same(got, splatio.unpack_splat_rows(rows, backend="torch"))
    q = {k: v[perm] for k, v in p.items()}
    assert torch.equal(got["means3d"], q["means3d"])                                    # positions are float32 in the file
    assert float((got["scales"] - q["scales"]).abs().max()) < 1e-5                      # exp, then log
    # a colour byte is trunc(255 v) read back as byte / 255: at most 1 / 255 below v (values inside [0, 1])
    rgb = q["features"][:, 0] * SH_C0 + 0.5
    inside = (rgb >= 0) & (rgb <= 1)
    assert float(((got["features"][:, 0] * SH_C0 + 0.5) - rgb)[inside].abs().max()) <= 1 / 255 * SLACK
    unit = q["quats"] / q["quats"].norm(dim=1, keepdim=True)
    assert float((got["quats"] - unit).abs().max()) <= 1 / 128 * SLACK                  # trunc(128 r + 128): a step of 1 / 128
    for bad in (0, 31, 65):
        open(path, "wb").write(bytes(bad))
        with pytest.raises(ValueError, match="multiple of 32"):
            ms.load_splat(path, backend="torch")


def _write_ply(path, header_lines, body):
    with open(path, "wb") as f:
        f.write(("\n".join(header_lines) + "\n").encode() + body)


def test_a_foreign_file_with_12_float_chunks_and_shuffled_properties_loads(tmp_path):
    """No colour bounds (they are 0 and 1), vertex words in another order with an extra property, a comment, an element
    after the ones that are read."""
    N = 300
    p = seeded_scene(N, 4, seed=6)
    cs = ms.compress_scene(p, order="keep", backend="torch")
    chunk12 = cs.chunks[:, :12].contiguous()
    names12 = splatio.CHUNK_PROPERTIES[:12]
    order = [2, 0, 3, 1]                                                                # file column -> which packed word
    vert = np.zeros(N, dtype=[("a", "<u4"), ("extra", "<f4"), ("b", "<u4"), ("c", "<u4"), ("d", "<u4")])
    words = cs.vertices.numpy().view(np.uint32)
    for col, wi in zip("abcd", order):
        vert[col] = words[:, wi]
    vnames = {"a": splatio.VERTEX_PROPERTIES[2], "b": splatio.VERTEX_PROPERTIES[0], "c": splatio.VERTEX_PROPERTIES[3],
              "d": splatio.VERTEX_PROPERTIES[1]}
    head = ["ply", "format binary_little_endian 1.0", "comment written by a test", "element chunk 2"] + \
        [f"property float {n}" for n in names12] + [f"element vertex {N}", f"property uint {vnames['a']}", "property float extra",
                                                     f"property uint {vnames['b']}", f"property uint {vnames['c']}",
                                                     f"property uint {vnames['d']}"] + \
        [f"element sh {N}"] + [f"property uchar f_rest_{i}" for i in range(9)] + ["element face 1", "property int tag", "end_header"]
    path = str(tmp_path / "foreign.ply")
    _write_ply(path, head, chunk12.numpy().tobytes() + vert.tobytes() + cs.sh.numpy().tobytes() + b"\0\0\0\0")
    got = ms.load_compressed_ply(path, backend="torch")
    want = ms.decompress_scene(ms.CompressedScene(chunk12, cs.vertices, cs.sh, None, 4), backend="torch")
    assert _same(got, want)
    full = ms.decompress_scene(cs, backend="torch")
    assert torch.equal(got["means3d"], full["means3d"]) and torch.equal(got["features"][:, 1:], full["features"][:, 1:])
    # colour bounds 0 and 1: rgb is the byte / 255 itself
    rgb = got["features"][:, 0] * SH_C0 + 0.5
    byte = torch.stack([(cs.vertices[:, 3] >> s) & 255 for s in (24, 16, 8)], 1).float() / 255
    assert float((rgb - byte).abs().max()) < 1e-6


def test_every_value_error(tmp_path):
    N, K = 300, 4
    p = seeded_scene(N, K, seed=7)
    cs = ms.compress_scene(p, backend="torch")
    good = expected_header(N, K).decode().splitlines()
    body = cs.chunks.numpy().tobytes() + cs.vertices.numpy().tobytes() + cs.sh.numpy().tobytes()
    path = str(tmp_path / "bad.ply")

    def load_raises(lines, data, match):
        _write_ply(path, lines, data)
        with pytest.raises(ValueError, match=match):
            ms.load_compressed_ply(path, backend="torch")

    load_raises([ln.replace("element chunk 2", "element chunk 3") for ln in good], body + bytes(72), "ceil")
    load_raises([ln.replace(f"element vertex {N}", "element vertex 0").replace("element chunk 2", "element chunk 0")
                 .replace(f"element sh {N}", "element sh 0") for ln in good], b"", "no Gaussian")
    load_raises([ln.replace("binary_little_endian", "ascii") for ln in good], body, "binary_little_endian")
    load_raises([ln.replace("binary_little_endian", "binary_big_endian") for ln in good], body, "binary_little_endian")
    load_raises([ln for ln in good if ln != "property float max_scale_y"], body, "max_scale_y")
    load_raises([ln for ln in good if ln != "property float max_g"], body, "max_g")
    load_raises([ln for ln in good if ln != "property uint packed_rotation"], body, "packed_rotation")
    load_raises([ln for ln in good if ln != "property uchar f_rest_8"], body, "f_rest")
    load_raises([ln.replace("property uint packed_scale", "property float packed_scale") for ln in good], body, "type")
    load_raises(good, body[:-1], "shorter")
    load_raises([ln for ln in good if not ln.startswith(("element chunk", "property float"))], body, "element chunk")
    # the params' checks are save_ply's
    with pytest.raises(ValueError, match="lacks"):
        ms.compress_scene({k: v for k, v in p.items() if k != "quats"}, backend="torch")
    with pytest.raises(ValueError, match="row counts"):
        ms.save_splat(path, {**p, "scales": p["scales"][:-1]}, backend="torch")
    with pytest.raises(ValueError, match="empty"):
        ms.save_compressed_ply(path, {k: v[:0] for k, v in p.items()}, backend="torch")
    for fn in (ms.compress_scene, lambda *a, **k: ms.save_splat(path, *a, **k)):
        with pytest.raises(ValueError, match="backend"):
            fn(p, backend="cuda")
        with pytest.raises(ValueError, match="opacity_space"):
            fn(p, opacity_space="log", backend="torch")
        with pytest.raises(ValueError, match="order"):
            fn(p, order="random", backend="torch")
    with pytest.raises(ValueError, match="order"):
        ms.compress_scene(p, order="importance", backend="torch")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        ms.compress_scene(p, backend="hip")
    # a CompressedScene that does not fit together
    with pytest.raises(ValueError, match="ceil"):
        ms.decompress_scene(cs._replace(chunks=cs.chunks[:1]), backend="torch")
    with pytest.raises(ValueError, match="sh must"):
        ms.decompress_scene(cs._replace(sh=None), backend="torch")
    with pytest.raises(ValueError, match="sh must"):
        ms.decompress_scene(cs._replace(K=9), backend="torch")
    with pytest.raises(ValueError, match="int32"):
        ms.decompress_scene(cs._replace(vertices=cs.vertices.long()), backend="torch")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        ms.decompress_scene(cs, backend="hip")


def test_a_failed_write_leaves_no_tmp_file(tmp_path, monkeypatch):
    p = seeded_scene(10, 1)
    path = str(tmp_path / "scene.ply")

    def refuse(src, dst):
        raise OSError("no rename today")

    monkeypatch.setattr(os, "replace", refuse)
    for save in (ms.save_compressed_ply, ms.save_splat):
        with pytest.raises(OSError, match="no rename"):
            save(path, p, backend="torch")
        assert not os.path.exists(path + ".tmp") and not os.path.exists(path)


def test_load_ply_still_refuses_a_compressed_file(tmp_path):
    """Unchanged behaviour: the INRIA loader reads files whose first element is the vertices."""
    path = str(tmp_path / "scene.compressed.ply")
    ms.save_compressed_ply(path, seeded_scene(10, 1), backend="torch")
    with pytest.raises(ValueError, match="comes before 'vertex'"):
        ms.load_ply(path, backend="torch")


def test_the_example_picks_its_loader_by_the_file(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import render_ply
    p = seeded_scene(10, 4)
    a, b, c = (str(tmp_path / n) for n in ("scene.ply", "scene.compressed.ply", "scene.SPLAT"))
    ms.save_ply(a, p, backend="torch")
    ms.save_compressed_ply(b, p, backend="torch")
    ms.save_splat(c, p, backend="torch")
    assert [render_ply.loader_for(x) for x in (a, b, c)] == [ms.load_ply, ms.load_compressed_ply, ms.load_splat]


def test_public_names_and_exported_symbols():
    for name in ("compress_scene", "decompress_scene", "save_compressed_ply", "load_compressed_ply", "save_splat", "load_splat"):
        assert name in ms.__all__ and getattr(ms, name) is getattr(splatio, name)
    assert ms.CompressedScene._fields == ("chunks", "vertices", "sh", "perm", "K")
    lib = _hip.load()
    for name in ("ms_splat_compress", "ms_splat_decompress", "ms_splat32_pack", "ms_splat32_unpack"):
        assert hasattr(lib, name) and name in _hip.EXPORTS


def test_c_abi_argument_validation():
    """The four entries validate before they touch the device (fake non-null pointers; nothing is dereferenced)."""
    L = _hip.load()
    P, Q = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)              # 16-byte aligned, and only 4-byte aligned
    N = ctypes.c_int64(10)
    OK, INVALID, TOO_LARGE = 0, 1, 3

    def err():
        return L.ms_last_error_string().decode()

    assert L.ms_splat_compress(ctypes.c_int64(-1), 1, P, P, P, P, None, P, P, None, None) == INVALID and "N < 0" in err()
    assert L.ms_splat_compress(ctypes.c_int64(0), 1, None, None, None, None, None, None, None, None, None) == OK
    assert L.ms_splat_compress(N, 0, P, P, P, P, None, P, P, None, None) == INVALID and "K = 0" in err()
    assert L.ms_splat_compress(N, 26, P, P, P, P, P, P, P, P, None) == INVALID and "K = 26" in err()
    assert L.ms_splat_compress(N, 1, None, P, P, P, None, P, P, None, None) == INVALID and "null" in err()
    assert L.ms_splat_compress(N, 4, P, P, P, P, None, P, P, P, None) == INVALID and "shr or sh" in err()
    assert L.ms_splat_compress(N, 1, P, Q, P, P, None, P, P, None, None) == INVALID and "16 bytes" in err()
    assert L.ms_splat_compress(N, 1, P, P, P, P, None, P, Q, None, None) == INVALID and "16 bytes" in err()
    assert L.ms_splat_compress(ctypes.c_int64(2 ** 40), 1, P, P, P, P, None, P, P, None, None) == TOO_LARGE
    assert L.ms_splat_decompress(ctypes.c_int64(-1), 1, 18, P, P, None, P, P, P, P, None, None) == INVALID and "N < 0" in err()
    assert L.ms_splat_decompress(ctypes.c_int64(0), 1, 18, None, None, None, None, None, None, None, None, None) == OK
    assert L.ms_splat_decompress(N, 1, 15, P, P, None, P, P, P, P, None, None) == INVALID and "chunk_floats = 15" in err()
    assert L.ms_splat_decompress(N, 4, 12, P, P, None, P, P, P, P, P, None) == INVALID and "shr or sh" in err()
    assert L.ms_splat_decompress(N, 1, 12, P, Q, None, P, P, P, P, None, None) == INVALID and "16 bytes" in err()
    assert L.ms_splat_decompress(N, 1, 18, P, P, None, None, P, P, P, None, None) == INVALID and "null" in err()
    for fn, args in ((L.ms_splat32_pack, [P, P, P, P, P]), (L.ms_splat32_unpack, [P, P, P, P, P])):
        assert fn(ctypes.c_int64(-1), *args, None) == INVALID and "N < 0" in err()
        assert fn(ctypes.c_int64(0), None, None, None, None, None, None) == OK
        assert fn(ctypes.c_int64(2 ** 40), *args, None) == TOO_LARGE
        for i in range(5):
            a = list(args)
            a[i] = None
            assert fn(N, *a, None) == INVALID and "null" in err()
    assert L.ms_splat32_pack(N, P, P, P, P, Q, None) == INVALID and "16 bytes" in err()
    assert L.ms_splat32_unpack(N, Q, P, P, P, P, None) == INVALID and "16 bytes" in err()
