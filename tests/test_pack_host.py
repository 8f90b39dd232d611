"""The oracle and the case table of tests/pack_cases.py, validated without a GPU: the array-built index map against the
element-by-element one, every case against the property it is named for, the derived reconstruction bound of the f16x3 split,
the exact inverse row scale, and every refusal of the pack entry points (they return before any launch)."""
import numpy as np
import pytest

import pack_cases as P


LOOP_BUDGET = 6000      # elements per (case, mode) that the element-by-element oracle visits


@pytest.mark.parametrize("c", P.X3_CASES + P.F16_CASES, ids=lambda c: type(c).__name__[:3] + "-" + c.name)
def test_vectorised_oracle_equals_loop_oracle(c):
    """every case's weight in all four `transposed` modes and both k orders (the d(columns) modes where the weight is 3x3, the
    chunk-major ones with the channels padded to a multiple of 32), the case's own padding or more: whole images where they
    are small, otherwise a spread of rows (first, last, the row padding) through the whole k range"""
    w = P.make_weight(c) if isinstance(c, P.X3Case) else P.make_weight_f16(c)
    O, I, R, S = w.shape
    own = (getattr(c, "korder", 0), c.transposed)
    modes = [(0, 0), (1, 0), (0, 1), (1, 1)]
    if (R, S) == (3, 3):
        modes += [(0, 2)] + ([(0, 3)] if I % 32 == 0 else [])
    assert own in modes
    for ko, t in modes:
        rows, chans, taps = P.packed_dims(O, I, R, S, t)
        chans_pad = c.chans_pad if (ko, t) == own else max(c.chans_pad, chans + 1)
        if ko == 1:
            chans_pad = -(-chans_pad // 32) * 32
        K = chans_pad if t >= 2 else taps * chans_pad
        rp, kp = rows + 2, K + 5
        n = max(4, LOOP_BUDGET // kp)
        pick = np.arange(rp) if rp <= n else np.unique(np.concatenate([np.linspace(0, rows - 1, n - 2).astype(int), [rows, rp - 1]]))
        vec = P.pack_image(w, O, I, R, S, chans_pad, rp, kp, ko, t)
        for row in pick:
            loop = np.array([P.pack_value_loop(w, O, I, R, S, chans_pad, ko, t, int(row), k) for k in range(kp)], np.float32)
            assert np.array_equal(vec[row].view(np.uint32), loop.view(np.uint32)), (c.name, ko, t, row)
        assert not vec[rows:].any() and not vec[:, K:].any()
    # the scalar / array entry point reads the same image
    (ko, t), (R, S) = own, (c.R, c.S)
    rows, chans, taps = P.packed_dims(c.O, c.I, c.R, c.S, t)
    K = c.chans_pad if t >= 2 else taps * c.chans_pad
    got = P.pack_value(w, c.O, c.I, c.R, c.S, c.chans_pad, ko, t, np.array([0, rows - 1, rows]), np.array([0, K - 1, K]))
    want = [P.pack_value_loop(w, c.O, c.I, c.R, c.S, c.chans_pad, ko, t, a, b) for a, b in ((0, 0), (rows - 1, K - 1), (rows, K))]
    assert np.array_equal(got, np.array(want, np.float32)) and want[2] == 0


def test_index_map_on_a_hand_written_weight():
    """a [2, 3, 2, 2] weight whose value spells its own index (o c r s as decimal digits), read back through every mode"""
    O, I, R, S = 2, 3, 2, 2
    w = np.fromfunction(lambda o, c, r, s: 1000 * o + 100 * c + 10 * r + s, (O, I, R, S)).astype(np.float32)
    pv = P.pack_value_loop
    assert pv(w, O, I, R, S, 4, 0, 0, 1, 2 * 4 + 2) == 1210          # forward: row o = 1, tap (1, 0), c = 2
    assert pv(w, O, I, R, S, 4, 0, 0, 1, 2 * 4 + 3) == 0             # channel padding
    assert pv(w, O, I, R, S, 4, 0, 0, 2, 0) == 0 and pv(w, O, I, R, S, 4, 0, 0, 0, 16) == 0     # row / tap padding
    assert pv(w, O, I, R, S, 2, 0, 1, 2, 1 * 2 + 1) == 1210          # input gradient: row c = 2, tap (0, 1) -> (1, 0), k-channel o = 1
    assert pv(w, O, I, R, S, 2, 0, 1, 0, 0) == 11 and pv(w, O, I, R, S, 2, 0, 1, 3, 0) == 0
    w9 = np.fromfunction(lambda o, c, r, s: 1000 * o + 10 * c + 3 * r + s, (2, 64, 3, 3)).astype(np.float32)
    assert pv(w9, 2, 64, 3, 3, 4, 0, 2, 5 * 64 + 40, 1) == 1000 + 400 + 5            # d(columns), tap-major rows
    assert pv(w9, 2, 64, 3, 3, 4, 0, 3, 288 + 5 * 32 + 8, 1) == 1000 + 400 + 5       # chunk-major rows: chunk 1, tap 5, c % 32 = 8
    assert pv(w9, 2, 64, 3, 3, 4, 0, 2, 0, 2) == 0 and pv(w9, 2, 64, 3, 3, 4, 0, 3, 576, 0) == 0
    assert pv(w9, 2, 64, 3, 3, 64, 1, 0, 1, (1 * 9 + 5) * 32 + 8) == 1000 + 400 + 5  # korder 1: chunk 1, tap 5, c % 32 = 8
    assert pv(w9, 2, 64, 3, 3, 64, 0, 0, 1, 5 * 64 + 40) == 1000 + 400 + 5           # korder 0


@pytest.mark.parametrize("c", P.X3_CASES, ids=lambda c: c.name)
def test_x3_case_reaches_its_edge(c):
    assert c.expect, c.name
    P.check_expect(c.expect, P.x3_properties(c))
    rows, chans, taps = P.packed_dims(c.O, c.I, c.R, c.S, c.transposed)
    assert c.rows_pad >= rows and c.chans_pad >= chans and 0 <= c.scale_n <= c.rows_pad
    assert (rows <= 64 or c.transposed >= 2) and c.layouts
    for layout in c.layouts:
        Kpad = P.x3_kpad(c, layout)
        img, scale = P.x3_image(P.make_weight(c), c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, Kpad, layout, c.transposed, c.scale_n)
        assert img.dtype == np.uint16 and img.shape == (c.rows_pad, 2 * Kpad) and scale.shape == (c.scale_n,)


@pytest.mark.parametrize("c", P.F16_CASES, ids=lambda c: c.name)
def test_f16_case_reaches_its_edge(c):
    assert c.expect, c.name
    P.check_expect(c.expect, P.f16_properties(c))
    w = P.make_weight_f16(c)
    img = P.f16_image(w, c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, c.Kpad, c.korder, c.transposed)
    assert img.dtype == np.uint16 and img.shape == (c.rows_pad, c.Kpad)
    if c.values:        # every planted value is in the image with the bits worked out by hand
        for j, (v, bits) in enumerate(c.values):
            o, rem = divmod(5 + j, c.I * 9)
            ch, tap = divmod(rem, 9)
            assert w[o, ch, tap // 3, tap % 3] == np.float32(v)
            assert img[o, tap * c.chans_pad + ch] == bits, (v, hex(img[o, tap * c.chans_pad + ch]), hex(bits))
        kinds = [b for _, b in c.values]
        assert 0x7C00 in kinds and 0xFC00 in kinds and 0x8000 in kinds and any(0 < b < 0x0400 for b in kinds)


def test_tables_cover_the_listed_modes():
    assert {c.transposed for c in P.X3_CASES} == {0, 1, 2, 3} == {c.transposed for c in P.F16_CASES}
    assert {l for c in P.X3_CASES for l in c.layouts} == {0, 2, 3, 5}
    assert {c.korder for c in P.F16_CASES} == {0, 1}
    assert {(c.layouts, c.transposed) for c in P.X3_CASES if c.transposed >= 2} == {((0, 5), 2), ((0, 5), 3)}
    assert any((c.R, c.S) == (7, 7) and c.I == 3 and c.chans_pad == 8 for c in P.X3_CASES)
    assert any(c.R != c.S for c in P.X3_CASES) and any(c.R != c.S for c in P.F16_CASES)
    assert any(c.O % 4 for c in P.X3_CASES if c.transposed == 0)
    pos = {k for c in P.X3_CASES for k in c.expect.get("amax_pos", {}).values()}
    assert {0, 63, 64, 255, 256, 287} <= pos
    assert len({c.name for c in P.X3_CASES}) == len(P.X3_CASES) and len({c.name for c in P.F16_CASES}) == len(P.F16_CASES)


def _rows_of_every_case():
    for c in P.X3_CASES:
        rows, chans, taps = P.packed_dims(c.O, c.I, c.R, c.S, c.transposed)
        K = c.chans_pad if c.transposed >= 2 else taps * c.chans_pad
        yield c, P.x3_rows(P.pack_image(P.make_weight(c), c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, K, 0, c.transposed))


def test_reconstruction_bound_and_exact_inverse_scale():
    """|hi + lo - v| <= 2^-13 (derived in pack_cases), 2^-23 of the row maximum where the cap did not act; pw * scale == 1 with
    both finite normal numbers, the subnormal maxima included; the scaled maximum lies in [1024, 2048) unless capped"""
    worst = worst_rel = 0.0
    tiny = np.finfo(np.float32).tiny
    for c, (v, hi, lo, pw, scale, sh, amax) in _rows_of_every_case():
        assert np.isfinite(v).all() and np.isfinite(hi.astype(np.float32)).all(), c.name
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64)).max(axis=1)
        assert (err <= P.RECON_BOUND).all(), (c.name, err.max())
        worst = max(worst, err.max())
        assert np.isfinite(pw).all() and np.isfinite(scale).all() and (pw >= tiny).all() and (scale >= tiny).all(), c.name
        assert (pw * scale == np.float32(1.0)).all() and (pw.astype(np.float64) * scale.astype(np.float64) == 1.0).all(), c.name
        assert (pw[amax == 0] == 1).all() and (scale[amax == 0] == 1).all()
        vmax = np.abs(v).max(axis=1)
        live = amax > 0
        uncapped = live & (11 - np.frexp(amax)[1] <= P.SHIFT_CAP)
        assert ((vmax[uncapped] >= 1024) & (vmax[uncapped] < 2048)).all(), c.name
        assert (vmax[live & ~uncapped] < 1024).all() and (vmax[live & ~uncapped] > 0).all(), c.name
        # the unscaled reconstruction scale * (hi + lo), relative to the row maximum
        rel = err[uncapped] / vmax[uncapped]
        assert (rel <= P.RECON_REL).all(), (c.name, rel.max())
        worst_rel = max(worst_rel, rel.max() if rel.size else 0.0)
    print(f"reconstruction: worst |hi + lo - v| = {worst:.3e} (bound {P.RECON_BOUND:.3e}), worst / row max = {worst_rel:.3e} "
          f"(bound {P.RECON_REL:.3e})")


def test_reconstruction_bound_on_random_rows():
    g = np.random.default_rng(5)
    img = (g.standard_normal((512, 288)) * np.exp(g.uniform(-60, 60, (512, 1)))).astype(np.float32)
    v, hi, lo, pw, scale, sh, amax = P.x3_rows(img)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))
    assert err.max() <= P.RECON_BOUND and (err.max(axis=1) / np.abs(v).max(axis=1)).max() <= P.RECON_REL
    back = (hi.astype(np.float64) + lo.astype(np.float64)) * scale.astype(np.float64)[:, None]
    assert (np.abs(back - img.astype(np.float64)).max(axis=1) <= P.RECON_REL * amax.astype(np.float64)).all()


def test_split_oracle_on_its_edge_image():
    a = P.split_edge_image()
    assert a.size % 4 == 0 and a.size // 4 > 256 and (a.size // 4) % 256 != 0 and not np.isnan(a).any()
    img = P.split_image(a)
    assert img.shape == (a.size // 4, 8) and img.dtype == np.uint16
    hi, lo = P.split(a)
    assert np.array_equal(img[:, :4].reshape(-1), hi.view(np.uint16)) and np.array_equal(img[:, 4:].reshape(-1), lo.view(np.uint16))
    assert np.isinf(hi.astype(np.float32)).any() and (hi.view(np.uint16) == 0x8000).any()
    assert ((lo.view(np.uint16) & 0x7FFF) < 0x0400).any() and ((lo.view(np.uint16) & 0x7FFF) > 0).any()


# ------------------------------------------------------------------------------------------------ refusals
W, OUT, SC = 0x10000, 0x20000, 0x30000          # never dereferenced: every call below is refused before a launch


def _x3_args(**kw):
    a = dict(w=W, packed=OUT, scale_out=SC, O=8, I=32, R=3, S=3, chans_pad=32, rows_pad=8, Kpad=288, layout=0, transposed=0, scale_n=8)
    a.update(kw)
    return [a[k] for k in ("w", "packed", "scale_out", "O", "I", "R", "S", "chans_pad", "rows_pad", "Kpad", "layout", "transposed",
                           "scale_n")] + [None]


_X3_REFUSALS = [
    ("null weight", dict(w=None), b"null pointer"),
    ("null output", dict(packed=None), b"null pointer"),
    ("null scale", dict(scale_out=None), b"null pointer"),
    ("layout 1", dict(layout=1), b"bad layout 1"),
    ("layout 4", dict(layout=4), b"bad layout 4"),
    ("layout 6", dict(layout=6), b"bad layout 6"),
    ("layout -1", dict(layout=-1), b"bad layout -1"),
    ("layout 0, Kpad % 4", dict(Kpad=290), b"not a multiple of 4"),
    ("layout 0, Kpad too small", dict(Kpad=284), b"Kpad=284 too small"),
    ("layout 3, wrong Kpad", dict(layout=3, Kpad=320), b"layout 3 needs"),
    ("layout 3, channels % 32", dict(layout=3, I=16, chans_pad=16, Kpad=144), b"layout 3 needs"),
    ("layout 3, not 3x3", dict(layout=3, R=1, S=1), b"layout 3 needs"),
    ("layout 2, wrong Kpad", dict(layout=2, Kpad=288), b"layout 2 needs"),
    ("layout 2, channels % 16", dict(layout=2, I=8, chans_pad=8, Kpad=80), b"layout 2 needs"),
    ("layout 2, not 3x3", dict(layout=2, R=3, S=1, Kpad=320), b"layout 2 needs"),
    ("layout 5, Kpad % 8", dict(layout=5, Kpad=292), b"layout 5 needs"),
    ("layout 5, Kpad too small", dict(layout=5, Kpad=280), b"layout 5 needs"),
    ("scale_n beyond rows_pad", dict(scale_n=9), b"scale_n=9 beyond rows_pad=8"),
    ("scale_n negative", dict(scale_n=-1), b"scale_n=-1"),
    ("misaligned output", dict(packed=OUT + 8), b"16-byte aligned"),
    ("chans_pad too small", dict(chans_pad=24, Kpad=216), b"padded sizes too small"),
    ("rows_pad too small", dict(rows_pad=7, scale_n=7), b"padded sizes too small"),
    ("input gradient, rows_pad < I", dict(transposed=1, rows_pad=16, scale_n=8), b"padded sizes too small"),
    ("input gradient, chans_pad < O", dict(transposed=1, O=40, rows_pad=32), b"padded sizes too small"),
    ("d(columns) with R = 3", dict(transposed=2, O=8, chans_pad=32, Kpad=32, rows_pad=288), b"d(columns)"),
    ("d(columns) in layout 3", dict(transposed=2, R=1, S=1, layout=3, chans_pad=32, Kpad=288, rows_pad=288), b"d(columns)"),
    ("d(columns) chunk-major, I % 32", dict(transposed=3, R=1, S=1, I=16, chans_pad=8, Kpad=8, rows_pad=144), b"d(columns)"),
    ("d(columns), rows_pad < 9 I", dict(transposed=2, R=1, S=1, chans_pad=8, Kpad=8, rows_pad=280), b"d(columns)"),
    ("d(columns), chans_pad < O", dict(transposed=3, R=1, S=1, O=16, chans_pad=8, Kpad=8, rows_pad=288), b"d(columns)"),
    ("transposed 4", dict(transposed=4, R=1, S=1, chans_pad=8, Kpad=8, rows_pad=288), b"d(columns)"),
]


@pytest.mark.parametrize("name,kw,msg", _X3_REFUSALS, ids=[r[0] for r in _X3_REFUSALS])
def test_pack_weights_x3_refusals(name, kw, msg):
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    assert l.ctdet_pack_weights_x3(*_x3_args(**kw)) == -22, name
    assert msg in l.ctdet_last_error(), (name, l.ctdet_last_error())
    assert b"pack_weights_x3" in l.ctdet_last_error()


def _f16_args(**kw):
    a = dict(w=W, packed=OUT, O=8, I=32, R=3, S=3, chans_pad=32, rows_pad=8, Kpad=288, korder=0, transposed=0)
    a.update(kw)
    return [a[k] for k in ("w", "packed", "O", "I", "R", "S", "chans_pad", "rows_pad", "Kpad", "korder", "transposed")] + [None]


_F16_REFUSALS = [
    ("null weight", dict(w=None), b"null pointer"),
    ("null output", dict(packed=None), b"null pointer"),
    ("chans_pad too small", dict(chans_pad=24), b"padded sizes too small"),
    ("rows_pad too small", dict(rows_pad=7), b"padded sizes too small"),
    ("Kpad too small", dict(Kpad=287), b"padded sizes too small"),
    ("input gradient, rows_pad < I", dict(transposed=1, rows_pad=16), b"padded sizes too small"),
    ("input gradient, chans_pad < O", dict(transposed=1, O=40, rows_pad=32), b"padded sizes too small"),
    ("chunk-major, channels % 32", dict(korder=1, I=16, chans_pad=16), b"chunk-major needs"),
    ("korder 2", dict(korder=2), b"chunk-major needs"),
    ("korder -1", dict(korder=-1), b"chunk-major needs"),
    ("d(columns), not 3x3", dict(transposed=2, R=1, S=1, chans_pad=8, Kpad=32, rows_pad=288), b"d(columns)"),
    ("d(columns), korder 1", dict(transposed=2, korder=1, chans_pad=32, Kpad=32, rows_pad=288), b"d(columns)"),
    ("d(columns), chans_pad < O", dict(transposed=2, O=16, chans_pad=8, Kpad=32, rows_pad=288), b"d(columns)"),
    ("d(columns), Kpad < chans_pad", dict(transposed=2, chans_pad=32, Kpad=24, rows_pad=288), b"d(columns)"),
    ("d(columns), rows_pad < 9 I", dict(transposed=2, chans_pad=8, Kpad=32, rows_pad=287), b"d(columns)"),
    ("d(columns) chunk-major, I % 32", dict(transposed=3, I=16, chans_pad=8, Kpad=32, rows_pad=144), b"d(columns)"),
    ("transposed 4", dict(transposed=4, chans_pad=8, Kpad=32, rows_pad=288), b"d(columns)"),
]


@pytest.mark.parametrize("name,kw,msg", _F16_REFUSALS, ids=[r[0] for r in _F16_REFUSALS])
def test_pack_weights_refusals(name, kw, msg):
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    assert l.ctdet_pack_weights(*_f16_args(**kw)) == -22, name
    assert msg in l.ctdet_last_error() and b"pack_weights:" in l.ctdet_last_error(), (name, l.ctdet_last_error())


@pytest.mark.parametrize("name,args,msg", [
    ("null source", (None, OUT, 16), b"bad arguments"),
    ("null destination", (W, None, 16), b"bad arguments"),
    ("negative n", (W, OUT, -4), b"bad arguments"),
    ("n % 4", (W, OUT, 18), b"multiple of 4 floats"),
    ("misaligned source", (W + 4, OUT, 16), b"16-byte aligned"),
    ("misaligned destination", (W, OUT + 8, 16), b"16-byte aligned"),
], ids=lambda a: a if isinstance(a, str) else "")
def test_split_weights_refusals(name, args, msg):
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    assert l.ctdet_split_weights(*args, None) == -22, name
    assert msg in l.ctdet_last_error() and b"split_weights" in l.ctdet_last_error(), (name, l.ctdet_last_error())


def test_batch_entry_points_refuse_bad_tables():
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    for fn, tag in ((l.ctdet_pack_weights_batch, b"pack_weights_batch"), (l.ctdet_pack_weights_x3_batch, b"pack_weights_x3_batch")):
        for args in ((None, 1, 1), (W, -1, 1), (W, 1, -1)):
            assert fn(*args, None) == -22 and tag in l.ctdet_last_error()
        assert fn(None, 0, 0, None) == 0 and fn(W, 0, 5, None) == 0 and fn(W, 3, 0, None) == 0        # nothing to do: no launch
