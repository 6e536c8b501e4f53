"""The training step's small kernels (csrc/elementwise.hip) on the MI355X, each driven directly through the C ABI and compared
by EQUALITY with its definition.

Every kernel here only adds, copies, or multiplies by values chosen as exact: the inputs are small integers (|x| <= 8, fewer than
2^21 terms) and dyadic fractions, so every partial sum in any order -- and every product, fused into the add or not -- is exactly
representable in fp32.  The expected result is the int64 / float64 evaluation of the definition cast to fp32, and a dropped,
doubled or misplaced element moves it by a whole unit; no summation order or FMA contraction can.

Every call gets fresh buffers of exactly the size the ABI documents (Buf): a canary behind each, workspaces and outputs that the
call must fill completely start as 0xFF bytes (a NaN in every float), gaps that the call must not touch are compared back."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAN = 1024   # canary bytes behind (and, for an offset buffer, in front of) every buffer
GAP = 4096.0  # what the padding between rows / slabs of an input holds: one of them in a sum is seen


class Buf:
    """A device buffer of exactly the bytes asked for: a numpy array's contents, or `init` bytes of 0xFF; random canary bytes
    behind it.  offset_words shifts the buffer by so many 4-byte words off the allocator's alignment."""

    def __init__(self, init, dtype=np.float32, offset_words=0):
        import torch
        assert torch.cuda.is_available(), "GPU tests need the MI355X"
        if isinstance(init, (int, np.integer)):
            self.nbytes, self.dtype, self.shape, host = int(init), np.dtype(dtype), None, None
        else:
            host = np.ascontiguousarray(init)
            self.nbytes, self.dtype, self.shape = host.nbytes, host.dtype, host.shape
        self.off = 4 * offset_words
        self.raw = torch.empty(self.off + self.nbytes + CAN, dtype=torch.uint8, device="cuda")
        self.canary = torch.randint(0, 256, (self.off + CAN,), dtype=torch.uint8, device="cuda")
        self.raw[:self.off] = self.canary[:self.off]
        self.raw[self.off + self.nbytes:] = self.canary[self.off:]
        if host is None:
            self.raw[self.off:self.off + self.nbytes] = 0xFF
        elif self.nbytes:
            self.raw[self.off:self.off + self.nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8)).cuda()
        self.ptr = self.raw.data_ptr() + self.off

    def get(self):
        import torch
        torch.cuda.synchronize()
        assert torch.equal(self.raw[:self.off], self.canary[:self.off]), "wrote in front of a buffer"
        assert torch.equal(self.raw[self.off + self.nbytes:], self.canary[self.off:]), "wrote behind a buffer"
        a = self.raw[self.off:self.off + self.nbytes].cpu().numpy().view(self.dtype)
        return a.reshape(self.shape) if self.shape is not None else a


def lib_and_stream():
    import torch
    import b2t_native as N
    return N.load(), torch.cuda.current_stream().cuda_stream


def ok(rc):
    import b2t_native as N
    assert rc == 0, N.last_error()


def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def same(got, want):
    """Equality of fp32 results with the float64 / int64 evaluation, which must itself be an fp32 value."""
    want = np.asarray(want)
    w32 = want.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want.astype(np.float64)), "the expected values are not exact in fp32"
    assert got.shape == w32.shape
    bad = np.flatnonzero(got.reshape(-1) != w32.reshape(-1))
    assert bad.size == 0, (bad.size, bad[:8], got.reshape(-1)[bad[:8]], w32.reshape(-1)[bad[:8]])


# ---- colsum ---------------------------------------------------------------------------------------------------------------
COLSUM = {   # rows, cols, ld, offset_words, Z, slab padding (x_sz - rows * ld), out padding (out_sz - cols)
    "vec4": (130, 260, 264, 0, 1, 0, 0),
    "cols_not_x4": (130, 41, 44, 0, 1, 0, 0),
    "ld_not_x4": (130, 64, 67, 0, 1, 0, 0),
    "x_off_one_word": (130, 64, 64, 1, 1, 0, 0),
    "long_rows": (4500, 72, 80, 0, 1, 0, 0),
    "rows_4096": (4096, 12, 12, 0, 1, 0, 0),
    "rows_4097": (4097, 12, 12, 0, 1, 0, 0),
    "z3_vec4": (130, 260, 264, 0, 3, 8, 12),
    "z3_x_sz_not_x4": (130, 260, 264, 0, 3, 5, 3),
}


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", sorted(COLSUM))
def test_colsum_every_path(case, accumulate):
    """b2t_colsum_f32: out[z out_sz + c] (+)= sum_r x[z x_sz + r ld + c] on the 16-byte path, on the scalar path for each of its
    reasons, on both sides of the 64 / 512 rows-per-block switch with the workspace exactly b2t_colsum_ws_bytes, batched with
    padded slabs; the padding of x never enters a sum, the padding of out is not written."""
    rows, cols, ld, offw, Z, xpad, opad = COLSUM[case]
    lib, st = lib_and_stream()
    rng = np.random.default_rng(sorted(COLSUM).index(case))
    x_sz, out_sz = rows * ld + xpad, cols + opad
    x = np.full((Z - 1) * x_sz + (rows - 1) * ld + cols, GAP, dtype=np.float32)
    val = ints(rng, (Z, rows, cols))
    for z in range(Z):
        for r in range(rows):
            x[z * x_sz + r * ld:z * x_sz + r * ld + cols] = val[z, r]
    out0 = ints(rng, (Z - 1) * out_sz + cols, -50, 50)
    need = lib.b2t_colsum_ws_bytes(rows, cols)
    assert need == -(-rows // (64 if rows <= 4096 else 512)) * cols * 4
    bx, bo, ws = Buf(x, offset_words=offw), Buf(out0), Buf(Z * need)
    ok(lib.b2t_colsum_f32(bx.ptr, rows, cols, ld, bo.ptr, accumulate, ws.ptr, Z, x_sz, out_sz, st))
    want = out0.astype(np.int64)
    for z in range(Z):
        s = val[z].astype(np.int64).sum(0)
        want[z * out_sz:z * out_sz + cols] = s + (want[z * out_sz:z * out_sz + cols] if accumulate else 0)
    same(bo.get(), want)
    ws.get(), bx.get()


# ---- slab_reduce ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1028, 2097152 + 12])
@pytest.mark.parametrize("nslab", [1, 7, 8, 9, 17])
def test_slab_reduce(nslab, n, accumulate):
    """b2t_slab_reduce_f32: out[i] (+)= sum_s slab[s n + i] with zero, one and two rounds of its eight-slab loop and every tail
    length class, at one block and where the grid-stride loop takes a second trip (n / 4 > 2048 x 256)."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(nslab * 3 + accumulate)
    slab = rng.integers(-8, 9, (nslab, n), dtype=np.int8)
    out0 = rng.integers(-50, 51, n).astype(np.float32)
    bs, bo = Buf(slab.astype(np.float32)), Buf(out0)
    ok(lib.b2t_slab_reduce_f32(bs.ptr, nslab, n, bo.ptr, accumulate, st))
    want = slab.sum(0, dtype=np.int64) + (out0.astype(np.int64) if accumulate else 0)
    same(bo.get(), want)


# ---- day_reduce -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("days,n,stride", [([3, 1, 3, 3, 1, 7, 3, 3, 3], 1028, 1040), ([2] * 1030, 4, 8)])
def test_day_reduce(days, n, stride):
    """b2t_day_reduce_f32: out[d stride + i] = sum over the day's sentences; a day of 1, 2 and 6 sentences (the four-at-a-time loop
    and its tail), rows of absent days and the padding between rows keep what they held, and 1030 sentences of one day: the
    tail behind the kernel's 1024-entry list."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(len(days))
    B, nd = len(days), max(days) + 1
    slab = ints(rng, (B, n))
    out0 = ints(rng, (nd - 1) * stride + n, -999, -900)
    bs, bd, bo = Buf(slab), Buf(np.array(days, dtype=np.int32)), Buf(out0)
    ok(lib.b2t_day_reduce_f32(bs.ptr, bd.ptr, B, n, bo.ptr, stride, st))
    want = out0.astype(np.int64)
    for d in sorted(set(days)):
        want[d * stride:d * stride + n] = slab[np.array(days) == d].astype(np.int64).sum(0)
    same(bo.get(), want)


# ---- cumsum_add / transpose / broadcast_rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("outer,n,inner", [(3, 50, 1), (2, 7, 33), (1, 1, 5)])
def test_cumsum_add(outer, n, inner):
    """b2t_cumsum_add_f32: y += cumsum(w) along the middle axis of [outer][n][inner], onto a prefilled y."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(n)
    w, y0 = ints(rng, (outer, n, inner)), ints(rng, (outer, n, inner), -50, 50)
    bw, by = Buf(w), Buf(y0)
    ok(lib.b2t_cumsum_add_f32(bw.ptr, by.ptr, outer, n, inner, st))
    same(by.get(), y0.astype(np.int64) + np.cumsum(w.astype(np.int64), axis=1))


@pytest.mark.parametrize("rows,cols", [(33, 65), (1, 100), (96, 32)])
def test_transpose(rows, cols):
    """b2t_transpose_f32 with every element a different value: partial tiles on both axes, one row, whole tiles."""
    lib, st = lib_and_stream()
    a = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols) - 1000.0
    bi, bo = Buf(a), Buf(rows * cols * 4)
    ok(lib.b2t_transpose_f32(bi.ptr, bo.ptr, rows, cols, st))
    same(bo.get().reshape(cols, rows), a.T.astype(np.float64))


def test_broadcast_rows():
    """b2t_broadcast_rows_f32: dst[b][0:n] = src[0:n], n no multiple of the block."""
    lib, st = lib_and_stream()
    rows, n = 5, 70
    src = np.arange(n, dtype=np.float32) * 3.0 - 100.0
    bs, bo = Buf(src), Buf(rows * n * 4)
    ok(lib.b2t_broadcast_rows_f32(bs.ptr, bo.ptr, rows, n, st))
    same(bo.get().reshape(rows, n), np.tile(src.astype(np.float64), (rows, 1)))


# ---- batch_gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 6, 8])
def test_batch_gather(W):
    """b2t_batch_gather_b32: out[b][t] = flat[row_off[b] + t] for t < min(lens[b], T_out), zeros behind; lengths 0, below, equal
    to and above T_out, row offsets in no order, a payload of arbitrary bit patterns (NaNs and infinities among them) compared as
    integers; the 4-byte path (W 1, 6) and the 16-byte path (W 8)."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(W)
    T_out, rows = 9, 60
    lens = np.array([0, 5, 9, 14, 1], dtype=np.int32)
    row_off = np.array([40, 3, 20, 46, 59], dtype=np.int64)
    B = len(lens)
    assert (row_off + lens <= rows).all()
    flat = rng.integers(0, 2 ** 32, (rows, W), dtype=np.uint64).astype(np.uint32)
    flat[7, 0], flat[22, W - 1] = 0x7FC00001, 0xFF800000
    bf, br, bl, bo = Buf(flat), Buf(row_off), Buf(lens), Buf(B * T_out * W * 4, dtype=np.uint32)
    ok(lib.b2t_batch_gather_b32(bf.ptr, br.ptr, bl.ptr, bo.ptr, B, T_out, W, st))
    want = np.zeros((B, T_out, W), dtype=np.uint32)
    for b in range(B):
        k = min(int(lens[b]), T_out)
        want[b, :k] = flat[row_off[b]:row_off[b] + k]
    assert np.array_equal(bo.get().reshape(B, T_out, W), want)


# ---- patch_fold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,patch,stride,F", [(61, 14, 4, 516), (30, 4, 2, 8), (20, 3, 5, 8), (17, 6, 1, 12)])
def test_patch_fold_is_the_definition(T, patch, stride, F):
    """b2t_patch_fold_f32 against du[b,t,f] = sum dv[b,p,k F + f] over p stride + k = t, written out as the scatter it is the
    adjoint of: overlapping windows, windows that tile T exactly, stride > patch (frames no window covers are exactly 0), stride
    1, and frames beyond the last window.  The fused day-layer backward is tested for bit identity with this kernel
    (tests/test_gpu_parity.py); this is the side that identity rests on."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(T)
    B, Tp = 2, (T - patch) // stride + 1
    dv = ints(rng, (B, Tp, patch, F))
    bv, bu = Buf(dv), Buf(B * T * F * 4)
    ok(lib.b2t_patch_fold_f32(bv.ptr, bu.ptr, B, T, F, Tp, patch, stride, st))
    want = np.zeros((B, T, F), dtype=np.int64)
    covered = np.zeros(T, dtype=bool)
    for p in range(Tp):
        for k in range(patch):
            want[:, p * stride + k] += dv[:, p, k].astype(np.int64)
            covered[p * stride + k] = True
    if (T, patch, stride) in ((61, 14, 4), (20, 3, 5)):
        assert not covered[-1], "the case is meant to have frames beyond the last window"
    if stride > patch:
        assert not covered[patch:stride].any()
    got = bu.get().reshape(B, T, F)
    same(got, want)
    assert not got[:, ~covered].any()


# ---- softsign_bwd -----------------------------------------------------------------------------------------------------------
def test_softsign_bwd():
    """b2t_softsign_bwd_f32: du *= (1 - |u|)^2 in place, u in sixteenths over [-1, 1] and integer du (every product exact), long
    enough that the grid-stride loop takes a second trip (n / 4 > 4096 x 256)."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(9)
    n = 4194304 + 8
    u = rng.integers(-16, 17, n).astype(np.float32) / 16.0
    du = ints(rng, n)
    u[:3], du[:3] = [1.0, -1.0, 0.0], [8.0, 8.0, 8.0]
    bu, bd = Buf(u), Buf(du)
    ok(lib.b2t_softsign_bwd_f32(bu.ptr, bd.ptr, n, st))
    same(bd.get(), du.astype(np.float64) * (1.0 - np.abs(u.astype(np.float64))) ** 2)
    assert np.array_equal(bu.get(), u)


# ---- augment_smooth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", [0, 1])
@pytest.mark.parametrize("ntaps", [5, 9, 33])
def test_augment_smooth_is_the_correlation(ntaps, padding):
    """b2t_augment_smooth_f32 with supplied noise against y[b,t,f] = sum_j taps[j] xn[b, t + j - left, f], xn = x[t + cut] +
    white_std white + offset_std offset, zero outside the cut sequence: the generic kernel (5 and 33 taps) and the windowed one
    (9), 'same' and 'valid' padding, cut > 0, three or four blocks along T with a partial last one, F = 516 (a second trip of the feature
    loop).  Integer x and noise, white_std 0.5, offset_std 0.25 and taps in sixteenths that are no palindrome: every term exact."""
    lib, st = lib_and_stream()
    rng = np.random.default_rng(ntaps + padding)
    B, T, F, cut = 2, 120, 516, 3
    Tc = T - cut
    T_out, left = (Tc, (ntaps - 1) // 2) if padding == 0 else (Tc - ntaps + 1, 0)
    assert T_out % 32 and T_out > 64
    taps = np.array([((5 * j) % 7 + 1) / 16.0 for j in range(ntaps)], dtype=np.float32)
    x, white, offset = ints(rng, (B, T, F)), ints(rng, (B, T, F), -4, 4), ints(rng, (B, F), -4, 4)
    bx, bw, bo, by = Buf(x), Buf(white), Buf(offset), Buf(B * T_out * F * 4)
    ok(lib.b2t_augment_smooth_f32(bx.ptr, by.ptr, B, T, F, cut, 0.5, 0.25, 1234, bw.ptr, bo.ptr,
                                  (C.c_float * ntaps)(*taps.tolist()), ntaps, padding, st))
    xn = np.zeros((B, Tc + 2 * ntaps, F))                      # the cut, noisy sequence with ntaps zeros on either side
    xn[:, ntaps:ntaps + Tc] = x[:, cut:].astype(np.float64) + 0.5 * white[:, cut:] + 0.25 * offset[:, None, :]
    want = np.zeros((B, T_out, F))
    for j in range(ntaps):
        want += float(taps[j]) * xn[:, ntaps + j - left:ntaps + j - left + T_out]
    same(by.get().reshape(B, T_out, F), want)
