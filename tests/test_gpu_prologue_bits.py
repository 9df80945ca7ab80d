"""The f16x2 weight pack and the whole-stack kernels' prologue, bit for bit: what the pack writes (pieces, fragment order, the
state's words), what the bias staging leaves in the on-chip bias table, and what the mixing prologue puts into the input panel."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

# Split16State as laid out in csrc/split16.h (byte offsets; the tests below cross-check them through Split16.read())
NT = 9
OFF_NPW, OFF_GEN, OFF_WFIRST, OFF_SA, OFF_SW, OFF_UPDATES, OFF_POISON, HEADER = 108, 120, 124, 176, 248, 324, 328, 408
CAP_WG, CAP_PW = 4096, 16384
OFF_PARTW = HEADER + 3 * CAP_WG * NT * 4
MAXL = 8
FILL = 0x5A


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def words(state):
    return state.buf.view(torch.int32)


def set_scales(state, off, values):
    state.buf[off:off + 4 * len(values)] = torch.tensor(np.asarray(values, np.float32).view(np.uint8), device="cuda")


# ---- the pack ------------------------------------------------------------------------------------------------------------------------
def ref_segment(Wlog, sc):
    """One segment as pack2_block documents it: dst[piece][cb][ki][lane] (16 B = 8 fp16) = piece(sc W[cb*16 + (lane&15)][ki*32 +
    (lane>>4)*8 .. +7]), hi = fp16(sc w), lo = fp16(sc w - hi), zero padded; and max |w| of every wave (= fragment)."""
    rows, cols = Wlog.shape
    ncb, kit = (rows + 15) // 16, (cols + 31) // 32
    P = np.zeros((ncb * 16, kit * 32), np.float32)
    P[:rows, :cols] = np.float32(sc) * Wlog
    hi = P.astype(np.float16)
    lo = (P - hi.astype(np.float32)).astype(np.float16)

    def frag(A):
        return A.reshape(ncb, 16, kit, 4, 8).transpose(0, 2, 3, 1, 4).reshape(-1)
    wmax = (np.abs(P) / np.float32(sc)).reshape(ncb, 16, kit, 32).max(axis=(1, 3)).reshape(-1)
    return frag(hi).view(np.uint8), frag(lo).view(np.uint8), wmax.astype(np.float32).view(np.uint32)


def ref_pack(Ws, scales):
    """Both destination buffers, the wave maxima of the forward segments, wfirst / nPW -- for layers Ws[l] of any shapes."""
    L = len(Ws)
    fwd, bwd, wmax, nwaves = [], [], [], [0]
    for l in range(L):
        h, lo, m = ref_segment(Ws[l], scales[l])
        fwd += [h, lo]; wmax.append(m); nwaves.append(nwaves[-1] + len(m))
    total = nwaves[-1]
    for l in range(L - 1, 0, -1):
        h, lo, m = ref_segment(np.ascontiguousarray(Ws[l].T), scales[l])
        bwd += [h, lo]; total += len(m)
    wfirst = [nwaves[min(l, L)] for l in range(NT + 1)]
    return np.concatenate(fwd), np.concatenate(bwd), np.concatenate(wmax), wfirst, total


# layers of one pack call; the entry point packs both orientations of a stack of L >= 2 layers, i.e. 2 L - 1 segments: 3 (the fewest),
# 5 and 15 = 2 MAXL - 1 (the most it can form; the argument block holds MAXSEG = 16).  Every shape runs forward, and -- when it is not
# the first of its list -- transposed.
PACK_LISTS = {
    "ragged-3seg": [(16, 32), (5, 3)],
    "ragged-5seg": [(5, 3), (16, 32), (17, 33)],
    "narrow": [(100, 10), (10, 100)],
    "wide": [(100, 10), (500, 100)],
    "maxseg": [(5, 3), (16, 32), (17, 33), (100, 10), (10, 100), (500, 100), (17, 33), (16, 32)],
}


def run_pack(ops, Ws_np, scales, merged, alarm=False):
    L = len(Ws_np)
    Ws = [dev(w) for w in Ws_np]
    st = ops.Split16(L, "cuda")
    set_scales(st, OFF_SW, scales)
    assert st.read()["scales_w"] == [float(s) for s in scales]          # the offsets above are the header's
    words(st)[OFF_PARTW // 4: OFF_PARTW // 4 + CAP_PW] = 0x5A5A5A5A
    sizing, sizing_t = ops.mlp_pack_split_both(Ws, None, None, state=ops.Split16(L, "cuda"))
    tail = 4096                                                          # sentinel bytes behind each buffer
    packed = torch.full((sizing.numel() + tail,), FILL, dtype=torch.uint8, device="cuda")
    packed_t = torch.full((sizing_t.numel() + tail,), FILL, dtype=torch.uint8, device="cuda")
    if merged:
        z, zt = torch.zeros(64, 10, device="cuda"), torch.zeros(64, 10, device="cuda")
        step = torch.tensor([3], dtype=torch.int32, device="cuda")
        ops.mlp_pack_split16_sample(Ws, packed, packed_t, st, "box", "uniform", "normal", 10, 64, z, zt, m_scale=1.0, c_scale=0.05,
                                    box=(0.0, 1.0), seed=11, stream_id=2, step_dev=step)
        torch.cuda.synchronize()
        assert float(z.abs().sum()) > 0 and float((zt - z).abs().sum()) > 0
    else:
        ops.mlp_pack_split_both(Ws, packed, packed_t, state=st)
        torch.cuda.synchronize()
    return packed.cpu().numpy(), packed_t.cpu().numpy(), words(st).cpu().numpy().view(np.uint32), tail


@pytest.mark.parametrize("merged", [False, True], ids=["pack2", "pack2+sample"])
@pytest.mark.parametrize("name", list(PACK_LISTS))
def test_pack2_bytes_state_words_and_sentinels(name, merged):
    """mlp_pack2_k and the merged front launch against a NumPy restatement, bytewise: both destination buffers (sentinels behind them
    untouched, padding zero), the forward waves' s16_partW slots (every other slot untouched), wfirst / nPW, the refreshed generation,
    and no poison.  Scales are powers of two, so sc w is exact and hi / lo are the two fp16 roundings."""
    from cl_ica_amd import ops
    shapes = PACK_LISTS[name]
    rng = np.random.default_rng(len(shapes) * 101 + shapes[0][0])
    Ws = [(rng.normal(size=s) * 0.1).astype(np.float32) for s in shapes]
    scales = [2.0 ** ((l % 4) - 1) * 4 for l in range(len(shapes))]
    want, want_t, wmax, wfirst, total_waves = ref_pack(Ws, scales)
    assert total_waves % 4 != 0, "the last block of the launch must be partly live"
    got, got_t, w, tail = run_pack(ops, Ws, scales, merged)
    assert got[:-tail].tobytes() == want.tobytes() and got_t[:-tail].tobytes() == want_t.tobytes()
    assert (got[-tail:] == FILL).all() and (got_t[-tail:] == FILL).all()
    pw = w[OFF_PARTW // 4: OFF_PARTW // 4 + CAP_PW]
    assert pw[:len(wmax)].tobytes() == wmax.tobytes()
    assert (pw[len(wmax):] == 0x5A5A5A5A).all()                          # transposed segments and dead waves record nothing
    assert list(w[OFF_WFIRST // 4: OFF_WFIRST // 4 + NT + 1]) == wfirst and w[OFF_NPW // 4] == wfirst[len(shapes)]
    assert w[OFF_GEN // 4] == w[OFF_UPDATES // 4] == 0
    assert w[OFF_POISON // 4] == 0xFFFFFFFF


@pytest.mark.parametrize("merged", [False, True], ids=["pack2", "pack2+sample"])
@pytest.mark.parametrize("name", list(PACK_LISTS))
def test_pack2_weight_beyond_the_alarm_in_the_last_segment_raises_poison(name, merged):
    """One weight of layer 1 -- the LAST segment (its transposed copy) holds it as well -- scaled past kF16Alarm: the poison word takes the
    generation (0 on a fresh state)."""
    from cl_ica_amd import ops
    shapes = PACK_LISTS[name]
    rng = np.random.default_rng(7)
    Ws = [(rng.normal(size=s) * 0.1).astype(np.float32) for s in shapes]
    scales = [4.0] * len(shapes)
    Ws[1][-1, -1] = 40000.0 / 4.0 * 1.5                                  # sc |w| = 60 000 > 32 768, still finite in fp16
    *_, w, _ = run_pack(ops, Ws, scales, merged)
    assert w[OFF_POISON // 4] == 0 == w[OFF_GEN // 4]


# ---- bias staging --------------------------------------------------------------------------------------------------------------------
BIAS_STACKS = {
    "3-5-2": [3, 5, 2],
    "headline": [10, 100, 500, 500, 100, 10],
    "maxl": [4, 8, 16, 24, 40, 8, 16, 5, 3],
    "sum480": [7, 200, 250], "sum512": [7, 224, 288], "sum544": [7, 200, 300],          # padded widths (multiples of 32) around 512 ...
    "sum992": [7, 500, 480], "sum1024": [7, 500, 500], "sum1056": [7, 500, 500, 20],    # ... and around 1024
    "no-bias-layer": [10, 100, 40, 10],
}


def bias_case(name):
    dims = BIAS_STACKS[name]
    L = len(dims) - 1
    assert L <= MAXL
    bs = []
    for l in range(L):
        i = np.arange(dims[l + 1], dtype=np.float32)
        bs.append(((-1.0) ** i * (1.0 + l + i / 1024.0)).astype(np.float32))       # distinct per (layer, feature), both signs, exact in fp32
    if name == "no-bias-layer":
        bs[1] = None
    want = []
    for l in range(L):
        b = np.zeros(dims[l + 1], np.float32) if bs[l] is None else bs[l]
        want.append(np.where(b > 0, b, np.float32(0.01) * b).astype(np.float32) if l < L - 1 else b)
    Ws = [torch.zeros(dims[l + 1], dims[l], device="cuda") for l in range(L)]
    x = dev(np.random.default_rng(1).normal(size=(50, dims[0])))          # 50 rows: two workgroups, the second with 2 live rows
    outs = [torch.full((50, d), float("nan"), device="cuda") for d in dims[1:]]
    return dims, Ws, [None if b is None else dev(b) for b in bs], x, outs, want


def check_bias_outs(outs, want, tag):
    for l, (o, b) in enumerate(zip(outs, want)):
        got = o.cpu().numpy()
        assert got.tobytes() == np.broadcast_to(b, got.shape).astype(np.float32).tobytes(), (tag, l)


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", list(BIAS_STACKS))
def test_zero_weights_leave_leaky_relu_of_the_bias_split(name, arith):
    """mlp_split_k with all weights zero: every saved layer output is LeakyReLU(bias) (the last layer: the bias) exactly, whatever the
    scales in force -- powers of two, and 1 for the last layer's output whatever the state says."""
    from cl_ica_amd import ops
    dims, Ws, bs, x, outs, want = bias_case(name)
    L = len(Ws)
    state = None
    if arith == "f16x2":
        state = ops.Split16(L, "cuda")
        sa = [2.0 ** ((t % 3) + 1) for t in range(L + 1)]
        set_scales(state, OFF_SA, sa)
        assert state.read()["scales_a"] == sa
    packed, _ = ops.mlp_pack_split_both(Ws, None, None, state=state)
    ops.mlp_fwd_split(x, Ws, bs, outs, packed, 0.01, signmasks=None, state=state)
    torch.cuda.synchronize()
    check_bias_outs(outs, want, arith)


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("name", list(BIAS_STACKS))
def test_zero_weights_leave_leaky_relu_of_the_bias_fp32(name, packed):
    """The same stacks through mlp_fwd_k, the native-fp32 whole-stack kernel."""
    from cl_ica_amd import ops
    dims, Ws, bs, x, outs, want = bias_case(name)
    ops.mlp_fwd(x, Ws, bs, outs, 0.01, packed=ops.mlp_pack_weights(Ws) if packed else None)
    torch.cuda.synchronize()
    check_bias_outs(outs, want, "fp32")


# ---- mixing prologue / input panel ---------------------------------------------------------------------------------------------------
def mix_case(n, mixL, seed=0):
    rng = np.random.default_rng(n * 13 + mixL + seed)
    dims = [n, 40, 72, n]
    L = len(dims) - 1
    Ws = [dev(rng.uniform(-1, 1, size=(dims[i + 1], dims[i])) / np.sqrt(dims[i])) for i in range(L)]
    bs = [dev(rng.uniform(-0.5, 0.5, size=dims[i + 1])) for i in range(L)]
    gW = dev(rng.normal(size=(mixL, n, n)) / np.sqrt(n))
    z = dev(rng.uniform(size=(50, n)))
    return dims, Ws, bs, gW, z


def fwd_mixed(ops, arith, dims, Ws, bs, gW, z, passes):
    L = len(Ws)
    M = z.shape[0]
    state = ops.Split16(L, "cuda") if arith == "f16x2" else None
    outs = [torch.empty(M, d, device="cuda") for d in dims[1:]]
    x_out = torch.full((M, dims[0]), float("nan"), device="cuda")
    packed = packed_t = None
    for _ in range(passes if state is not None else 1):                   # f16x2: the scales settle on the data first
        packed, packed_t = ops.mlp_pack_split_both(Ws, packed, packed_t, state=state)
        ops.mlp_fwd_split(z, Ws, bs, outs, packed, 0.01, signmasks=None, mix=(gW, 0.2, x_out), state=state)
        if state is not None:
            state.update()
    torch.cuda.synchronize()
    return x_out, outs


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("mixL", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 10, 16])
def test_fused_mixing_prologue_xout_equals_the_mixing_kernel(n, mixL, arith):
    """x = g(z) as the fused forward's prologue computes and stores it == clica_mixing_fwd, bit for bit (n up to MIX_MAX_N = 16)."""
    from cl_ica_amd import ops
    dims, Ws, bs, gW, z = mix_case(n, mixL)
    x_ref = ops.mixing_fwd(z, gW, 0.2)
    x_out, _ = fwd_mixed(ops, arith, dims, Ws, bs, gW, z, passes=1)
    assert x_out.cpu().numpy().tobytes() == x_ref.cpu().numpy().tobytes()


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_fused_mixing_forward_matches_fp64(arith):
    """One mixed forward at n = 10 against fp64 under the stack tests' rule (1e-5 of the largest element): a padding column of the input
    panel left unzeroed (the corner the mixing net worked in holds its intermediates and weights) would show up here."""
    from cl_ica_amd import ops
    dims, Ws, bs, gW, z = mix_case(10, 3, seed=5)
    x_out, outs = fwd_mixed(ops, arith, dims, Ws, bs, gW, z, passes=4)
    a = x_out.cpu().numpy().astype(np.float64)
    for l in range(len(Ws)):
        a = a @ Ws[l].cpu().numpy().astype(np.float64).T + bs[l].cpu().numpy().astype(np.float64)
        if l < len(Ws) - 1:
            a = np.where(a > 0, a, 0.01 * a)
        assert rel_err(outs[l].cpu().numpy(), a) < 1e-5, (arith, l)
