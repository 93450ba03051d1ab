"""Fusion-buffer pack/unpack (batched_copy_k) and the Adasum combine
(adasum_dots_k / adasum_scaledadd_k) on the GPU, at the edges.

Pack/unpack.  On one rank RCCL's reduction is the identity, so the output of a
collective is exactly unpack(pack(x)) and the expected value is computed bit
for bit on the CPU.  With T the tensor dtype, W the wire dtype and A = fp64 if
T or W is fp64, else fp32 (the scale itself is rounded to A):

    wire = cast_W( cast_A(x)    * cast_A(pre)  )
    out  = cast_T( cast_A(wire) * cast_A(post) )

Every comparison is bit equality on integer views, so NaN and -0.0 count; no
tolerance is used anywhere.  One input rule makes that achievable: in the
cases that convert fp64 to a 2-byte wire the inputs are fp32-representable
and the prescale is a power of two, because torch's CPU cast rounds
fp64 -> fp32 -> fp16 while the device may round once; with such inputs the two
agree.  Groups hold at least two tensors: a single unscaled same-dtype tensor
takes the direct RCCL path and never reaches the pack kernel.  Tensors hold
distinct values (_values), so a shifted or duplicated chunk, or a value from a
neighbouring tensor, fails the equality check itself; 1- and 2-byte types
cannot hold 300 001 distinct values and repeat with their full period.

int16 GPU tensors travel as int32 (RCCL has no 16-bit integer type).

Not covered, and not to be called on the GPU: a scale other than 1 on integer
tensors, and groups that mix integer dtypes.  BatchedCopyLaunch returns
hipErrorInvalidValue for both and the error is raised on the background
thread.

Adasum combine, through _core.adasum_combine_.  The reference is fp64 on CPU
copies of the inputs, which are already rounded to their dtype: dot, na, nb in
fp64, ac = 1 - dot/(2 na) (1 if na == 0), bc likewise from nb, and
ref = ac*a + bc*b.  Per element

    |got - ref| <= u_T*|ref| + n * 2^-50 * (|a_i| + |b_i|)

with u_T = 2^-53 (fp64), 2^-24 (fp32), 2^-11 + 2^-24 (fp16) and
2^-8 + 2^-24 (bf16); the extra 2^-24 is the fp32 step the kernel takes on the
way down, and the second term is the worst case of the unordered fp64 atomic
sums.  Both terms are derived, not measured.  b is rescaled to a's norm, so
|a|/|b| is within [1/2, 2] and the second term holds as written.  fp16
operands are drawn at scale 256 so that no |ref| falls below 2^-14, where
fp16 rounds absolutely (2^-25) rather than relatively; the test asserts this
about its own inputs.  Each case prints its worst error / bound.

The exact cases (b = a, b = -a) need dot, na and nb to be summed in the same
order; the sums are atomic across blocks, and a sum of at most two non-zero
block partials does not depend on the order, so these cases run at n <= 1024
on aligned operands, where at most two blocks hold data.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [1, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000]
BIG = 300001  # > 256 blocks x 256 threads x VS: the grid-stride loop repeats
INTS = [torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8,
        torch.bool]
FLOATS = [torch.float64, torch.float32, torch.float16, torch.bfloat16]
SCALES = [(2.0, 0.25), (1.0 / 3.0, 3.0 / 7.0)]
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_names = itertools.count()


@pytest.fixture(scope="module")
def hvd():
    import horovod_amd.torch as hvd
    hvd.init()
    torch.cuda.set_device(0)
    yield hvd
    # process-level shutdown handled by atexit


def _name(tag):
    return f"pack.{tag}.{next(_names)}"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT_VIEW[t.element_size()])


def _assert_bits(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, \
        (what, got.dtype, exp.dtype, got.shape, exp.shape)
    g, e = _bits(got).flatten(), _bits(exp).flatten()
    bad = (g != e).nonzero().flatten()
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.numel()} of {g.numel()} elements differ, first at "
            f"{i}: got {got.flatten()[i].item()!r} (bits {int(g[i]):#x}), "
            f"expected {exp.flatten()[i].item()!r} (bits {int(e[i]):#x})")


def _values(n, dtype, k):
    """n distinct finite values of `dtype` (CPU), different for every k; the
    integers lie above 2^24 and the fp64 ones are not fp32-representable"""
    i = torch.arange(n, dtype=torch.int64)
    if dtype == torch.int64:
        return i + (k + 1) * 2**40 + 1
    if dtype == torch.int32:
        return (i + (k + 1) * 2**24 + 1).to(dtype)
    if dtype == torch.float64:
        return i.double() + k * 2**20 + 1.0 / 3.0
    if dtype == torch.float32:
        return (i + k * 2**20).float() * 0.5
    if dtype == torch.int16:
        return ((i + 7919 * k) % 65536 - 32768).to(dtype)
    if dtype == torch.float16:   # the bit patterns of the positive normals
        return (0x0400 + (i + 7919 * k) % 0x7800).to(torch.int16).view(dtype)
    if dtype == torch.bfloat16:
        return (0x0080 + (i + 7919 * k) % 0x7F00).to(torch.int16).view(dtype)
    if dtype == torch.uint8:
        return ((i + 37 * k) % 256).to(dtype)
    if dtype == torch.int8:
        return ((i + 37 * k) % 256 - 128).to(dtype)
    assert dtype == torch.bool
    return (i * (k + 3)) % 3 == 0


def _expected(x, wire, pre, post):
    """The formula of the module docstring, on a CPU tensor"""
    if not x.dtype.is_floating_point:
        assert pre == 1.0 and post == 1.0
        return x.clone()
    if wire == x.dtype and pre == 1.0 and post == 1.0:
        return x.clone()  # a bit copy: the NaN keeps its payload
    acc = torch.float64 if torch.float64 in (x.dtype, wire) else torch.float32
    w = (x.to(acc) * torch.tensor(pre, dtype=acc)).to(wire)
    return (w.to(acc) * torch.tensor(post, dtype=acc)).to(x.dtype)


def _grouped(hvd, xs, tag, pre=1.0, post=1.0, compression=None, wire=None):
    """grouped_allreduce of CPU tensors xs on the GPU against the formula;
    the wire is tensors[0]'s dtype unless compression sets it"""
    wire = wire or xs[0].dtype
    outs = hvd.grouped_allreduce([x.cuda() for x in xs], average=False,
                                 name=_name(tag), compression=compression,
                                 prescale_factor=pre, postscale_factor=post)
    assert len(outs) == len(xs)
    for j, (x, o) in enumerate(zip(xs, outs)):
        _assert_bits(o, _expected(x, wire, pre, post),
                     f"{tag} tensor {j} ({x.dtype}, n={x.numel()})")


# ---- same-type exactness ---------------------------------------------------

def _int_specials(dtype):
    info = torch.iinfo(dtype)
    cand = [0, 1, -1, 2**24 + 1, -(2**24 + 1), 2**31 - 1, -2**31, 2**40 + 1,
            -(2**40 + 1), 2**62 + 1, info.min, info.max]
    return torch.tensor([v for v in cand if info.min <= v <= info.max],
                        dtype=dtype)


def _float_specials(dtype):
    info = torch.finfo(dtype)
    return torch.tensor([float("inf"), float("-inf"), float("nan"), -0.0, 0.0,
                         info.smallest_normal * info.eps,  # least subnormal
                         -info.smallest_normal * info.eps, info.max, info.min,
                         info.smallest_normal, 1.0], dtype=dtype)


@pytest.mark.parametrize("dtype", INTS + FLOATS, ids=str)
def test_same_type_pack_is_bit_copy(hvd, dtype):
    """An unscaled same-dtype group comes back bit for bit.  Before the
    convert_only fix the copy went through fp32: int64 and int32 lost
    everything above 2^24 and fp64 came back with fp32 precision."""
    if dtype == torch.bool:
        special = torch.tensor([True, False, False, True, True, False, True])
    elif dtype == torch.float64:
        g = torch.Generator().manual_seed(40)
        special = torch.cat([_float_specials(dtype),
                             torch.randn(37, dtype=dtype, generator=g)])
        assert not torch.equal(special[11:], special[11:].float().double())
    elif dtype.is_floating_point:
        special = _float_specials(dtype)
    else:
        special = _int_specials(dtype)
    _grouped(hvd, [special, _values(37, dtype, 1), _values(8, dtype, 2)],
             f"same.{dtype}")


# ---- sizes, the vector/tail split and the second grid-stride trip -----------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32,
                                   torch.int64, torch.float16, torch.uint8],
                         ids=str)
def test_sizes_and_grid_stride(hvd, dtype):
    xs = [_values(n, dtype, k) for k, n in enumerate(SMALL + [BIG])]
    _grouped(hvd, xs, f"sizes.{dtype}")


# ---- misaligned operands ---------------------------------------------------

def _views(dtype, device):
    """(buffer, view) pairs on `device`: contiguous views at element offsets
    1, 2 and 3 into a larger buffer, sizes around the vector width"""
    pairs = []
    for k, (off, n) in enumerate([(1, 1000), (2, 17), (3, 64), (1, 9),
                                  (3, 65)]):
        buf = _values(n + 8, dtype, k).to(device)
        pairs.append((buf, buf[off:off + n], off))
    return pairs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64,
                                   torch.float16, torch.int32, torch.uint8],
                         ids=str)
def test_misaligned_source(hvd, dtype):
    """Pack from views that are not 16-byte aligned (vec_ok false)"""
    pairs = _views(dtype, "cuda")
    outs = hvd.grouped_allreduce([v for _, v, _ in pairs], average=False,
                                 name=_name(f"missrc.{dtype}"))
    for j, ((buf, v, off), o) in enumerate(zip(pairs, outs)):
        assert v.data_ptr() % 16 != 0 or dtype == torch.float64 and off == 2
        _assert_bits(o, v.cpu(), f"missrc {dtype} tensor {j}")


@pytest.mark.parametrize(
    "dtype,pre,post",
    [(dt, pre, post) for dt in FLOATS for pre, post in [(1.0, 1.0)] + SCALES] +
    [(torch.int32, 1.0, 1.0), (torch.uint8, 1.0, 1.0)],
    ids=lambda v: str(v) if isinstance(v, torch.dtype) else f"{v:.3g}")
def test_misaligned_inplace(hvd, dtype, pre, post):
    """grouped_allreduce_ on the views: misaligned pack source and unpack
    destination; the guard elements around each view stay as they were"""
    pairs = _views(dtype, "cuda")
    expected = []
    for buf, v, off in pairs:
        e = buf.cpu().clone()
        e[off:off + v.numel()] = _expected(v.cpu(), dtype, pre, post)
        expected.append(e)
    hvd.grouped_allreduce_([v for _, v, _ in pairs], average=False,
                           name=_name(f"misinp.{dtype}"),
                           prescale_factor=pre, postscale_factor=post)
    for j, ((buf, v, off), e) in enumerate(zip(pairs, expected)):
        _assert_bits(buf, e, f"misinp {dtype} buffer {j} (view at {off})")


# ---- descriptor batches ----------------------------------------------------

@pytest.mark.parametrize("dtype,pre,post",
                         [(torch.float32, 1.0, 1.0),
                          (torch.float32, 1.0 / 3.0, 3.0 / 7.0),
                          (torch.int64, 1.0, 1.0),
                          (torch.bfloat16, 2.0, 0.25)],
                         ids=["f32", "f32-thirds", "i64", "bf16-pow2"])
def test_fifty_tensors_cross_descriptor_batch(hvd, dtype, pre, post):
    """50 tensors > kCopyBatchCapacity = 48: two launches per direction"""
    xs = [_values(SMALL[k % len(SMALL)], dtype, k) for k in range(50)]
    _grouped(hvd, xs, f"fifty.{dtype}", pre, post)


@pytest.mark.parametrize("pre,post", [(1.0, 1.0)] + SCALES,
                         ids=["unscaled", "pow2", "thirds"])
def test_mixed_float_group(hvd, pre, post):
    """[fp32, bf16, fp32, fp16]: the wire is tensors[0]'s fp32 and
    PackEntries flushes at every dtype change; each output keeps its dtype"""
    dts = [torch.float32, torch.bfloat16, torch.float32, torch.float16]
    g = torch.Generator().manual_seed(41)
    xs = [torch.randn(n, generator=g).to(dt)
          for dt, n in zip(dts, [65, 1000, 17, 63])]
    _grouped(hvd, xs, "mixed", pre, post, wire=torch.float32)


# ---- scale and conversion --------------------------------------------------

@pytest.mark.parametrize("pre,post", SCALES, ids=["pow2", "thirds"])
@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_scaled_group(hvd, dtype, pre, post):
    g = torch.Generator().manual_seed(42)
    xs = [torch.randn(n, dtype=torch.float64, generator=g).to(dtype)
          for n in (1000, 7, 65, 16)]
    if dtype == torch.float64:
        assert not torch.equal(xs[0], xs[0].float().double())
    _grouped(hvd, xs, f"scaled.{dtype}", pre, post)


def _compressible(dtype, seed):
    """fp32-representable values (see the input rule in the docstring)"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype) for n in (1000, 9, 64, 17)]


@pytest.mark.parametrize("wire", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_compressed_group_and_single(hvd, dtype, wire):
    """fp32 / fp64 tensors over an fp16 / bf16 wire with the power-of-two
    scale pair, as a group and as one compressed hvd.allreduce"""
    from horovod_amd.torch.compression import Compression
    comp = Compression.fp16 if wire == torch.float16 else Compression.bf16
    pre, post = SCALES[0]
    xs = _compressible(dtype, 43)
    _grouped(hvd, xs, f"comp.{dtype}.{wire}", pre, post, compression=comp,
             wire=wire)
    x = xs[0]
    out = hvd.allreduce(x.cuda(), average=False, compression=comp,
                        name=_name("comp1"), prescale_factor=pre,
                        postscale_factor=post)
    _assert_bits(out, _expected(x, wire, pre, post),
                 f"single compressed allreduce {dtype} over {wire}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_reducescatter_prescale(hvd, dtype):
    g = torch.Generator().manual_seed(44)
    x = torch.randn(1001, generator=g).to(dtype)
    out = hvd.reducescatter(x.cuda(), op=hvd.Sum, prescale_factor=3.0,
                            name=_name("rs"))
    _assert_bits(out, _expected(x, dtype, 3.0, 1.0),
                 f"reducescatter {dtype}")


# ---- Adasum combine --------------------------------------------------------

ADA_N = [1, 7, 8, 9, 1024, 65537]
U = {torch.float64: 2.0**-53, torch.float32: 2.0**-24,
     torch.float16: 2.0**-11 + 2.0**-24, torch.bfloat16: 2.0**-8 + 2.0**-24}


def _ada_pair(n, dtype, seed, rho=0.3):
    """a, b of `dtype` on the CPU with correlation ~rho and equal norms"""
    g = torch.Generator().manual_seed(seed)
    scale = 256.0 if dtype == torch.float16 else 1.0
    a = torch.randn(n, dtype=torch.float64, generator=g) * scale
    b = rho * a + (1 - rho * rho) ** 0.5 * scale * torch.randn(
        n, dtype=torch.float64, generator=g)
    b = b * (a.norm() / b.norm())
    return a.to(dtype), b.to(dtype)


def _ada_ref(a, b):
    ad, bd = a.double(), b.double()
    dot, na, nb = ad.dot(bd), ad.dot(ad), bd.dot(bd)
    ac = 1.0 - dot / (2.0 * na) if na > 0 else torch.tensor(1.0).double()
    bc = 1.0 - dot / (2.0 * nb) if nb > 0 else torch.tensor(1.0).double()
    return ac * ad + bc * bd, float(ac), float(bc)


def _ada_ratio(got, a, b):
    """worst |got - ref| / bound over the elements of one pair"""
    ref, _, _ = _ada_ref(a, b)
    n = a.numel()
    if a.double().norm() > 0 and b.double().norm() > 0:
        r = float(a.double().norm() / b.double().norm())
        assert 0.5 <= r <= 2.0, r
    nonzero = ref[ref != 0].abs()
    if a.dtype == torch.float16 and nonzero.numel():
        assert float(nonzero.min()) >= 2.0**-14, "test inputs"
    bound = U[a.dtype] * ref.abs() + n * 2.0**-50 * (a.double().abs() +
                                                     b.double().abs())
    err = (got.cpu().double() - ref).abs()
    assert torch.isfinite(got.cpu().double()).all()
    # err <= bound everywhere, zero bound included
    return float(torch.where(err == 0, torch.zeros_like(err),
                             err / bound).max())


def _combine(a_list, b_list):
    from horovod_amd import _core
    _core.adasum_combine_(a_list, b_list)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_adasum_against_fp64(hvd, dtype):
    pairs = [_ada_pair(n, dtype, 50 + i) for i, n in enumerate(ADA_N)]
    ga = [a.cuda() for a, _ in pairs]
    gb = [b.cuda() for _, b in pairs]
    _combine(ga, gb)
    for (a, b), got, gbk in zip(pairs, ga, gb):
        ratio = _ada_ratio(got, a, b)
        print(f"adasum {dtype} n={a.numel()}: worst error / bound = "
              f"{ratio:.3g}")
        assert ratio <= 1.0, (dtype, a.numel(), ratio)
        _assert_bits(gbk, b, f"adasum b untouched {dtype} n={a.numel()}")


def _ada_view(x, off):
    """x on the GPU as a view at element offset `off` into a larger buffer
    (off = 0: aligned); returns the buffer and the view"""
    pad = torch.full((4,), 7.0, dtype=x.dtype)
    buf = torch.cat([pad[:off], x, pad]).cuda()
    return buf, buf[off:off + x.numel()]


@pytest.mark.parametrize("off_a,off_b", [(1, 0), (0, 3), (1, 3)],
                         ids=["a+1", "b+3", "a+1,b+3"])
@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_adasum_on_views(hvd, dtype, off_a, off_b):
    """a and b as views at element offsets 1 and 3, one misaligned at a time
    and then both: the unvectorised path.  The elements of a's buffer around
    the view, and all of b's buffer, stay as they were"""
    worst = 0.0
    for i, n in enumerate([9, 1000]):
        a, b = _ada_pair(n, dtype, 60 + i)
        bufa, va = _ada_view(a, off_a)
        bufb, vb = _ada_view(b, off_b)
        before_a, before_b = bufa.cpu().clone(), bufb.cpu().clone()
        _combine([va], [vb])
        worst = max(worst, _ada_ratio(va, a, b))
        _assert_bits(bufb, before_b, "adasum b buffer untouched")
        _assert_bits(bufa[:off_a], before_a[:off_a], "guard before a")
        _assert_bits(bufa[off_a + n:], before_a[off_a + n:], "guard after a")
    print(f"adasum views {dtype} a+{off_a} b+{off_b}: worst error / bound = "
          f"{worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_adasum_zero_vectors(hvd, dtype):
    """A zero norm gives a coefficient of exactly 1 and no NaN: a = 0 leaves
    b*bc = b, b = 0 leaves a*ac = a, both zero leave zero"""
    for n in (1, 9, 1024):
        a, b = _ada_pair(n, dtype, 70 + n)
        z = torch.zeros(n, dtype=dtype)
        ga = [z.cuda(), a.cuda(), z.cuda()]
        gb = [b.cuda(), z.cuda(), z.cuda()]
        _combine(ga, gb)
        _assert_bits(ga[0], b, f"a = 0, {dtype} n={n}")
        _assert_bits(ga[1], a, f"b = 0, {dtype} n={n}")
        _assert_bits(ga[2], z, f"a = b = 0, {dtype} n={n}")


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_adasum_equal_and_opposite(hvd, dtype):
    """b = a gives a exactly (ac = bc = 1/2); b = -a gives 0 exactly
    (ac = bc = 3/2, and the two rounded products cancel)"""
    for n in (1, 7, 8, 9, 1024):
        a, _ = _ada_pair(n, dtype, 80 + n)
        ga = [a.cuda(), a.cuda()]
        gb = [a.cuda(), (-a).cuda()]
        _combine(ga, gb)
        _assert_bits(ga[0], a, f"b = a, {dtype} n={n}")
        assert torch.equal(ga[1].cpu(), torch.zeros(n, dtype=dtype)), \
            (f"b = -a, {dtype} n={n}", ga[1].cpu().double().abs().max())
        _assert_bits(gb[1], -a, "b untouched")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_adasum_fifty_pairs(hvd, dtype):
    """50 pairs > 48 descriptors: two launches per stage.  Every pair has its
    own correlation, so a dots slot used for another tensor fails the bound"""
    sizes = [1, 7, 8, 9, 64, 257]
    pairs = [_ada_pair(sizes[k % len(sizes)], dtype, 100 + k,
                       rho=-0.9 + 1.8 * k / 49) for k in range(50)]
    ga = [a.cuda() for a, _ in pairs]
    gb = [b.cuda() for _, b in pairs]
    _combine(ga, gb)
    worst = 0.0
    for k, ((a, b), got, gbk) in enumerate(zip(pairs, ga, gb)):
        ratio = _ada_ratio(got, a, b)
        assert ratio <= 1.0, (k, a.numel(), ratio)
        worst = max(worst, ratio)
        _assert_bits(gbk, b, f"pair {k}: b untouched")
    print(f"adasum 50 pairs {dtype}: worst error / bound = {worst:.3g}")
