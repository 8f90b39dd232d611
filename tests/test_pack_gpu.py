"""The weight-packing kernels (pack_weights_kernel, pack_weights_batch_kernel, pack3_kernel, pack3_batch_kernel,
split_weights_kernel) through the C ABI against the numpy oracle of tests/pack_cases.py (validated on the CPU by
tests/test_pack_host.py).  Every comparison is of bits.  Every output starts as sentinels (f16 0x7C01, a signalling NaN no
conversion produces; f32 0x7FC12345) with guard elements behind it: the image must be overwritten everywhere, the guards and
scale_out[scale_n:] must keep their sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_cases as P

pytestmark = pytest.mark.gpu

H_SENT, F_SENT = 0x7C01, 0x7FC12345
GUARD = 64


@pytest.fixture(scope="module")
def L(dev):
    from detectron2_centernet_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _halves(n, dev):
    return torch.full((n,), H_SENT, dtype=torch.int16, device=dev)


def _words(n, dev):
    return torch.full((n,), F_SENT, dtype=torch.int32, device=dev)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {first}: got {int(got[first]):#06x}, "
                             f"oracle {int(want[first]):#06x}; rows {sorted({int(b[0]) for b in bad})[:12]}")


def pack_f16(L, wd, c, dev):
    """one ctdet_pack_weights launch of case c -> uint16 [rows_pad, Kpad]; guards checked"""
    _lib, l = L
    n = c.rows_pad * c.Kpad
    out = _halves(n + GUARD, dev)
    _lib.check(l.ctdet_pack_weights(wd.data_ptr(), out.data_ptr(), c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, c.Kpad, c.korder,
                                    c.transposed, _stream()), "ctdet_pack_weights")
    got = _u16(out)
    assert (got[n:] == H_SENT).all(), f"{c.name}: written past rows_pad * Kpad"
    assert (got[:n] != H_SENT).all(), f"{c.name}: {(got[:n] == H_SENT).sum()} elements of the image were not written"
    return got[:n].reshape(c.rows_pad, c.Kpad)


def pack_x3(L, wd, dims, layout, transposed, scale_n, dev, name=""):
    """one ctdet_pack_weights_x3 launch -> (uint16 [rows_pad, 2 Kpad], uint32 scale bits [scale_n]); guards checked"""
    _lib, l = L
    O, I, R, S, chans_pad, rows_pad, Kpad = dims
    n = rows_pad * 2 * Kpad
    out, sc = _halves(n + GUARD, dev), _words(scale_n + GUARD, dev)
    _lib.check(l.ctdet_pack_weights_x3(wd.data_ptr(), out.data_ptr(), sc.data_ptr(), O, I, R, S, chans_pad, rows_pad, Kpad, layout,
                                       transposed, scale_n, _stream()), "ctdet_pack_weights_x3")
    got, gs = _u16(out), _u32(sc)
    assert (got[n:] == H_SENT).all(), f"{name} layout {layout}: written past rows_pad * Kpad"
    assert (gs[scale_n:] == F_SENT).all(), f"{name} layout {layout}: scale_out written at or past scale_n"
    assert (got[:n] != H_SENT).all(), f"{name} layout {layout}: {(got[:n] == H_SENT).sum()} halves of the image were not written"
    assert (gs[:scale_n] != F_SENT).all(), f"{name} layout {layout}: scale_out not written below scale_n"
    return got[:n].reshape(rows_pad, 2 * Kpad), gs[:scale_n]


def _dims(c, layout):
    return (c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, P.x3_kpad(c, layout))


# ------------------------------------------------------------------------------------------------ single launches
@pytest.mark.parametrize("c", P.F16_CASES, ids=lambda c: c.name)
def test_pack_weights_f16_bits(L, dev, c):
    w = P.make_weight_f16(c)
    got = pack_f16(L, _dev(w, dev), c, dev)
    _same(got, P.f16_image(w, c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, c.Kpad, c.korder, c.transposed), c.name)


@pytest.mark.parametrize("c", P.X3_CASES, ids=lambda c: c.name)
def test_pack_weights_x3_bits(L, dev, c):
    """image and scale of every layout of the case, as bits; the scale first: a wrong row scale explains a wrong row"""
    w = P.make_weight(c)
    wd = _dev(w, dev)
    for layout in c.layouts:
        dims = _dims(c, layout)
        got, gs = pack_x3(L, wd, dims, layout, c.transposed, c.scale_n, dev, c.name)
        want, ws = P.x3_image(w, *dims, layout, c.transposed, c.scale_n)
        bad = np.flatnonzero(gs != ws.view(np.uint32))
        assert bad.size == 0, (f"{c.name} layout {layout}: scale_out differs in rows {bad[:8].tolist()}: got "
                               f"{[hex(int(x)) for x in gs[bad[:8]]]}, oracle {[hex(int(x)) for x in ws.view(np.uint32)[bad[:8]]]}")
        _same(got, want, f"{c.name} layout {layout}")


def test_split_weights_bits(L, dev):
    _lib, l = L
    a = P.split_edge_image()
    src, dst = _dev(a, dev), _halves(2 * a.size + GUARD, dev)
    _lib.check(l.ctdet_split_weights(src.data_ptr(), dst.data_ptr(), a.size, _stream()), "ctdet_split_weights")
    got = _u16(dst)
    assert (got[2 * a.size:] == H_SENT).all() and (got[:2 * a.size] != H_SENT).all()
    _same(got[:2 * a.size].reshape(-1, 8), P.split_image(a), "split image")
    assert np.array_equal(_u32(src.view(torch.int32)), a.view(np.uint32)), "the source image was changed"


# ------------------------------------------------------------------------------------------------ non-finite weights
def test_pack_weights_x3_non_finite_rows(L, dev):
    """a NaN, a +inf and a -inf, one row each: every other row is the oracle's, and the planted element's hi half is not finite in
    every layout (the optimizer step's finite guard reads the packed operands' effect, not the parameter); the remaining bits of
    those three rows are not pinned"""
    c = P.x3_case("k288_second_amax_pass")
    w = P.make_weight(c)
    plants = [(1, 100, np.float32(np.nan)), (2, 257, np.float32(np.inf)), (6, 3, np.float32(-np.inf))]
    rows = [r for r, _, _ in plants]
    for r, k, v in plants:
        tap, ch = divmod(k, c.I)
        w[r, ch, tap // 3, tap % 3] = v
    clean = w.copy()
    clean[rows] = 1.0
    keep = np.setdiff1d(np.arange(c.rows_pad), rows)
    wd = _dev(w, dev)
    for layout in c.layouts:
        dims = _dims(c, layout)
        got, gs = pack_x3(L, wd, dims, layout, 0, c.scale_n, dev, "non-finite")
        want, ws = P.x3_image(clean, *dims, layout, 0, c.scale_n)
        _same(got[keep], want[keep], f"layout {layout}, rows without a non-finite weight")
        assert np.array_equal(gs[keep], ws.view(np.uint32)[keep])
        for r, k, v in plants:
            mark = np.zeros_like(w)                      # where does the oracle put the hi half of (row, k)?
            tap, ch = divmod(k, c.I)
            mark[r, ch, tap // 3, tap % 3] = 1.0
            at = np.flatnonzero(P.x3_image(mark, *dims, layout, 0, c.scale_n)[0][r] == 0x6400)
            assert at.size == 1
            assert got[r, at[0]] & 0x7C00 == 0x7C00, f"layout {layout}: hi of {v} at row {r} is {int(got[r, at[0]]):#06x}"


# ------------------------------------------------------------------------------------------------ batch kernels
def _table(arr, dev):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _place(sizes, align, gap):
    """offsets of buffers of `sizes` elements in one allocation: `gap` guard elements in front of, between and behind them"""
    offs, at = [], gap
    for n in sizes:
        offs.append(at)
        at = -(-(at + n + gap) // align) * align
    return offs, at


F16_BATCH = ("forward_3x3_tap_major", "non_square_3x1", "input_gradient_chunk_major", "dcn_cols_chunk_major", "one_by_one",
             "f16_edge_values")


def test_pack_weights_batch_equals_single_launches(L, dev):
    _lib, l = L
    cases = [P.f16_case(n) for n in F16_BATCH]
    mods = [c.rows_pad * c.Kpad % 256 for c in cases]
    assert 0 in mods and any(mods), mods                         # a last block that is full, and partly idle ones
    ws = [P.make_weight_f16(c) for c in cases]
    wds = [_dev(w, dev) for w in ws]
    singles = [pack_f16(L, wd, c, dev) for wd, c in zip(wds, cases)]
    sizes = [c.rows_pad * c.Kpad for c in cases]
    offs, total = _place(sizes, 8, 24)
    for ncases in (len(cases), 1):                               # the binary search over n descriptors, and over one
        out = _halves(total, dev)
        arr = (_lib.PackDesc * ncases)()
        blk = 0
        for d, c, wd, off in zip(arr, cases, wds, offs):
            d.w, d.packed = wd.data_ptr(), out.data_ptr() + 2 * off
            d.O, d.I, d.R, d.S, d.chans_pad, d.rows_pad, d.Kpad, d.korder, d.transposed = (
                c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, c.Kpad, c.korder, c.transposed)
            d.blk0 = blk
            blk += (c.rows_pad * c.Kpad + 255) // 256
        table = _table(arr, dev)
        _lib.check(l.ctdet_pack_weights_batch(table.data_ptr(), ncases, blk, _stream()), "ctdet_pack_weights_batch")
        first = _u16(out).copy()
        written = np.zeros(total, bool)
        for c, w, single, off, n in list(zip(cases, ws, singles, offs, sizes))[:ncases]:
            _same(first[off:off + n].reshape(single.shape), single, f"batch of {ncases}: {c.name} against its single launch")
            _same(single, P.f16_image(w, c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, c.Kpad, c.korder, c.transposed), c.name)
            written[off:off + n] = True
        assert (first[~written] == H_SENT).all(), f"batch of {ncases}: the gaps between the outputs were written"
        _lib.check(l.ctdet_pack_weights_batch(table.data_ptr(), ncases, blk, _stream()), "ctdet_pack_weights_batch")
        assert np.array_equal(_u16(out), first), "a second identical launch changed the bytes"


X3_BATCH = (("k288_second_amax_pass", 3), ("layout2_one_chunk", 2), ("one_by_one", 0), ("dcn_cols_chunk_major_i32", 5),
            ("scale_n_below_rows_pad", 5), ("amax_f32_max", 0), ("scale_n_zero", 0), ("amax_2^-149_smallest_subnormal", 5))


def test_pack_weights_x3_batch_equals_single_launches(L, dev):
    _lib, l = L
    items = [(P.x3_case(n), layout) for n, layout in X3_BATCH]
    assert {layout for _, layout in items} == {0, 2, 3, 5} and len({c.rows_pad for c, _ in items}) >= 4
    ws = [P.make_weight(c) for c, _ in items]
    wds = [_dev(w, dev) for w in ws]
    singles = [pack_x3(L, wd, _dims(c, layout), layout, c.transposed, c.scale_n, dev, c.name) for wd, (c, layout) in zip(wds, items)]
    sizes = [c.rows_pad * 2 * P.x3_kpad(c, layout) for c, layout in items]
    offs, total = _place(sizes, 8, 24)
    soffs, stotal = _place([c.scale_n for c, _ in items], 1, 5)
    for nitems in (len(items), 1):
        out, sc = _halves(total, dev), _words(stotal, dev)
        arr = (_lib.Pack3Desc * nitems)()
        blk = 0
        for d, (c, layout), wd, off, soff in zip(arr, items, wds, offs, soffs):
            d.w, d.packed, d.scale_out = wd.data_ptr(), out.data_ptr() + 2 * off, sc.data_ptr() + 4 * soff
            d.O, d.I, d.R, d.S, d.chans_pad, d.rows_pad, d.Kpad, d.layout, d.transposed, d.scale_n = (
                c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, P.x3_kpad(c, layout), layout, c.transposed, c.scale_n)
            d.blk0 = blk
            blk += c.rows_pad
        table = _table(arr, dev)
        _lib.check(l.ctdet_pack_weights_x3_batch(table.data_ptr(), nitems, blk, _stream()), "ctdet_pack_weights_x3_batch")
        first, fs = _u16(out).copy(), _u32(sc).copy()
        written, swritten = np.zeros(total, bool), np.zeros(stotal, bool)
        for (c, layout), w, (img, gs), off, n, soff in list(zip(items, ws, singles, offs, sizes, soffs))[:nitems]:
            _same(first[off:off + n].reshape(img.shape), img, f"batch of {nitems}: {c.name} layout {layout} against its single launch")
            assert np.array_equal(fs[soff:soff + c.scale_n], gs), f"batch of {nitems}: {c.name} scale"
            want, wsc = P.x3_image(w, *_dims(c, layout), layout, c.transposed, c.scale_n)
            _same(img, want, f"{c.name} layout {layout}")
            assert np.array_equal(gs, wsc.view(np.uint32))
            written[off:off + n] = True
            swritten[soff:soff + c.scale_n] = True
        assert (first[~written] == H_SENT).all(), f"batch of {nitems}: the gaps between the images were written"
        assert (fs[~swritten] == F_SENT).all(), f"batch of {nitems}: the gaps between the scales were written"
        _lib.check(l.ctdet_pack_weights_x3_batch(table.data_ptr(), nitems, blk, _stream()), "ctdet_pack_weights_x3_batch")
        assert np.array_equal(_u16(out), first) and np.array_equal(_u32(sc), fs), "a second identical launch changed the bytes"


# ------------------------------------------------------------------------------------------------ the torch chain
CHAIN_CASES = [c for c in P.X3_CASES if c.transposed == 0]


def _chain_rows(amax):
    """rows inside the torch chain's documented range: 1e-30 <= amax, the maximum not within one ulp of a power of two (its
    floor(log2()) in f32 is not to be trusted there)"""
    amax = np.asarray(amax, np.float32)
    m, _ = np.frexp(amax)
    near = (m == np.float32(0.5)) | (m == np.nextafter(np.float32(0.5), np.float32(1))) | (m == np.nextafter(np.float32(1), np.float32(0)))
    return (amax >= np.float32(1e-30)) & ~near


@pytest.mark.parametrize("c", CHAIN_CASES, ids=lambda c: c.name)
def test_pack_weights_x3_agrees_with_the_torch_chain(L, dev, c):
    """PackedConv on an f64 weight takes the torch chain (permute / pad / row maximum / exp2(10 - floor(log2)) / ctdet_split_weights
    / _pack_pairs); inside that chain's range the kernel's layouts 0, 2 and 3 and its scale are the same bits"""
    import detectron2_centernet_amd.ops as ops
    w = P.make_weight(c)
    wd = _dev(w, dev)
    ref = ops.PackedConv(wd.double(), None, None, stride=1, pad=c.R // 2, compute=ops.F16X3, cin_pad=c.chans_pad)
    assert ref._x3_src is None and ref.Cin == c.chans_pad
    rows_pad, Kpad, scale_n = ref.Cout_pad, ref.Kpad, ref.Cout_eff
    amax = np.zeros(max(rows_pad, 32 * -(-rows_pad // 32)), np.float32)
    amax[:c.O] = np.abs(w.reshape(c.O, -1)).max(axis=1)
    ok = _chain_rows(amax)
    assert ok[:c.O].any(), c.name
    got, gs = pack_x3(L, wd, (c.O, c.I, c.R, c.S, c.chans_pad, rows_pad, Kpad), 0, 0, scale_n, dev, c.name)
    chain = _u16(ref.w.view(torch.int16).reshape(rows_pad, 2 * Kpad))
    _same(got[ok[:rows_pad]], chain[ok[:rows_pad]], f"{c.name}: layout 0 against the torch chain")
    assert np.array_equal(gs[ok[:scale_n]], _u32(ref.scale.view(torch.int32))[ok[:scale_n]]), f"{c.name}: scale against the torch chain"
    if ref._wp_scaled is not None:
        img, korder = ref._pack_pairs(ref._wp_scaled)
        assert korder == (3 if (c.chans_pad // 16) % 2 == 0 else 2)
        prow, pK = img.shape[0], img.shape[1]
        gotp, _ = pack_x3(L, wd, (c.O, c.I, c.R, c.S, c.chans_pad, prow, pK), korder, 0, scale_n, dev, c.name)
        chainp = _u16(img.contiguous().view(torch.int16).reshape(prow, 2 * pK))
        _same(gotp[ok[:prow]], chainp[ok[:prow]], f"{c.name}: layout {korder} against the torch chain")
    else:
        assert (c.R, c.S) != (3, 3) or c.chans_pad % 16
