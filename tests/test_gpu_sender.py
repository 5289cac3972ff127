"""GPU tests of the fused sender (include/ldpc_erasure_amd_sender.h): source symbols on the device straight to FEC wire packets.

The expected bytes are built WITHOUT the code under test: codewords from the CPU oracle (oracle.OracleCode.encode, per frame),
laid out in numpy as [F*n][8+S] with the header word of api.fec_header_pack.  On top of that: which path ran (fused kernel or
encode + packetise through a bounded scratch), guard bands around the output at three alignments, equality with what the
library already offers, the block counter of FecTxDevice, the whole device pipeline sender -> channel -> reassembler ->
decode_frames, and the argument errors."""
import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, ENOCODE, EUNSUP = -1, -4, -5
MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def heavy_code(n=48, k=24, rowdeg=22, seed=5):
    """A small triangular code whose source columns sit in most checks: column degrees above 16, which the scatter encoder
    does not take (the sender then goes through the gather encoder and the packetiser)."""
    rng = np.random.default_rng(seed)
    m = n - k
    H = np.zeros((m, n), dtype=np.uint8)
    for i in range(m):
        c = rng.choice(k + i, size=min(rowdeg - 1, k + i), replace=False)
        H[i, c] = rng.integers(1, 256, size=c.size)
        H[i, k + i] = rng.integers(1, 256)
    code = codes.from_dense(H, k)
    assert np.bincount(code.cols, minlength=n).max() > 16
    return code


def non_triangular_code():
    """n = 12, k = 6: row r ends at column n - 1 - r, not at k + r -- no systematic encoder."""
    n, k = 12, 6
    H = np.zeros((n - k, n), dtype=np.uint8)
    for r in range(n - k):
        H[r, r] = 1 + r
        H[r, (r + 1) % k] = 7 + r
        H[r, n - 1 - r] = 3
    return codes.from_dense(H, k)


_CODES = {}


def get_code(ctx, which):
    """(handle, codes.Code) of built-in code 0 / 1 / 3 or of the heavy-column code ("heavy"), registered once per module."""
    if which not in _CODES:
        if which == "heavy":
            code = heavy_code()
            _CODES[which] = (ctx.register_code(code), code)
        else:
            _CODES[which] = (ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
    return _CODES[which]


def make_source(F, k, S, seed):
    return torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=_gen(seed))


def oracle_packets(oracle, code, src_host, fec_class, block0):
    """[F*n][8+S] from the CPU oracle's codewords and api.fec_header_pack (host arithmetic): nothing of the device path."""
    F, k, S = src_host.shape
    oc = oracle.OracleCode(code)
    n = code.n
    pk = np.zeros((F * n, 8 + S), dtype=np.uint8)
    for f in range(F):
        cw = oc.encode(src_host[f, :, 0]) if S == 1 else oc.encode(src_host[f])
        pk[f * n:(f + 1) * n, 8:] = cw.reshape(n, S)
        for j in range(n):
            pk[f * n + j, :8] = np.frombuffer(api.fec_header_pack(fec_class, (block0 + f) & 0xFF, j).to_bytes(8, "little"), dtype=np.uint8)
    return pk


def send(ctx, h, src, fec_class, block0, out=None):
    return ctx.fec_encode_packets_device(h, src[:, :, 0].contiguous() if src.shape[2] == 1 else src, fec_class, block0, out=out)


# ------------------------------------------------------------------------------------------ 1. bytes against the oracle
# (code, S, F, fec_class, block0): every code / S pair of the list at F in {1, 3, 70}; F = 260 at S = 16 wraps the block number;
# block0 = 250 wraps it too; both header classes
CASES = [
    (1, 1024, 3, 1, 0), (1, 1024, 70, 0xAB, 250), (1, 1024, 1, 1, 5),
    (1, 128, 70, 1, 0), (1, 128, 1, 0xAB, 7), (1, 128, 3, 1, 255),
    (1, 16, 260, 1, 0), (1, 16, 3, 0xAB, 250),
    (1, 1, 70, 1, 0), (1, 1, 1, 0xAB, 250), (1, 1, 3, 1, 254),
    (3, 1024, 3, 0xAB, 0), (3, 1024, 70, 1, 250), (3, 1024, 1, 1, 0),
    (3, 16, 70, 1, 0), (3, 16, 1, 0xAB, 255),
    (0, 256, 3, 1, 0), (0, 256, 70, 0xAB, 250), (0, 256, 1, 1, 9),
    ("heavy", 128, 3, 1, 0), ("heavy", 128, 70, 0xAB, 250), ("heavy", 128, 1, 1, 0),
]


@pytest.mark.parametrize("which,S,F,fec_class,block0", CASES)
def test_packets_equal_oracle_built_packets(ctx, oracle, which, S, F, fec_class, block0):
    h, code = get_code(ctx, which)
    src = make_source(F, code.k, S, seed=1000 + 7 * S + F)
    want = oracle_packets(oracle, code, src.cpu().numpy(), fec_class, block0)
    fresh = send(ctx, h, src, fec_class, block0)
    ctx.synchronize()
    assert tuple(fresh.shape) == (F * code.n, 8 + S)
    assert np.array_equal(fresh.cpu().numpy(), want), "fresh buffer"
    filled = torch.full((F * code.n, 8 + S), 0x5A, dtype=torch.uint8, device="cuda")
    got = send(ctx, h, src, fec_class, block0, out=filled)
    ctx.synchronize()
    assert got.data_ptr() == filled.data_ptr()
    assert np.array_equal(filled.cpu().numpy(), want), "buffer pre-filled with 0x5A"


# ------------------------------------------------------------------------------------------ 2. the path is the one promised
@pytest.mark.parametrize("which,S", [(1, 1024), (3, 1024), (1, 128)])
def test_default_knobs_take_the_fused_kernel(which, S):
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        assert c.knobs() == ""
        assert c.fec_sender_info() == {"path": "none", "scratch_bytes": 0}
        h = c.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which])
        n, k, _ = c.code_info(h)
        src = make_source(4, k, S, seed=S + which)
        for _ in range(2):
            c.fec_encode_packets_device(h, src)
        c.synchronize()
        assert c.fec_sender_info()["path"] == "fused"
        assert c.fec_sender_info()["scratch_bytes"] == 0          # a fused-only sequence allocates no codeword scratch
        assert "ldpc_scatter_static_pkt_kernel" in c.profile_kernel_names()["apply"]


def test_s1_and_knob_zero_take_the_composed_path_with_the_same_bytes():
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        h = c.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        n, k, _ = c.code_info(h)
        c.fec_encode_packets_device(h, make_source(3, k, 1, seed=1)[:, :, 0].contiguous())
        assert c.fec_sender_info()["path"] == "composed"
        src = make_source(5, k, 1024, seed=2)
        fused = c.fec_encode_packets_device(h, src, 3, 254)
        assert c.fec_sender_info()["path"] == "fused"
        c.configure("LDPC_AMD_ENC_PKT", 0)
        assert "ENC_PKT=0" in c.knobs()
        composed = c.fec_encode_packets_device(h, src, 3, 254)
        assert c.fec_sender_info()["path"] == "composed"
        c.synchronize()
        assert torch.equal(fused, composed)
        c.configure("LDPC_AMD_ENC_PKT", None)
        assert c.knobs() == ""
        c.fec_encode_packets_device(h, src, 3, 254)
        assert c.fec_sender_info()["path"] == "fused"


def test_composed_scratch_is_bounded():
    """F = 600 frames of (2040,1530) at S = 1024 are 1.25 GB of codewords: the composed path goes through them in chunks."""
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        h = c.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        n, k, _ = c.code_info(h)
        F, S = 600, 1024
        src = make_source(F, k, S, seed=3)
        fused = c.fec_encode_packets_device(h, src, 1, 100)
        c.configure("LDPC_AMD_ENC_PKT", 0)
        composed = c.fec_encode_packets_device(h, src, 1, 100)
        info = c.fec_sender_info()
        c.synchronize()
        assert info["path"] == "composed" and 0 < info["scratch_bytes"] <= 256 * MIB
        assert F * n * S > 256 * MIB                               # (so several chunks ran, each with its own first block number)
        assert torch.equal(fused, composed)
        want = c.fec_packetize_device(c.encode(h, src), 1, 100)
        c.synchronize()
        assert torch.equal(composed, want)


# ------------------------------------------------------------------------------------------ 3. guard bands
@pytest.mark.parametrize("S", [1024, 128])
def test_guard_bands_at_three_alignments(ctx, oracle, S):
    h, code = get_code(ctx, 1)
    F, G = 3, 4096
    src = make_source(F, code.k, S, seed=40 + S)
    want = oracle_packets(oracle, code, src.cpu().numpy(), 1, 17)
    nbytes = F * code.n * (8 + S)
    for shift, must_be in ((0, "fused"), (8, None), (1, "composed")):
        big = torch.full((G + 16 + nbytes + G + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        start = G + (-(big.data_ptr() + G) % 16) + shift              # 16-byte aligned, then + shift
        assert (big.data_ptr() + start) % 16 == shift
        out = big[start:start + nbytes].view(F * code.n, 8 + S)
        ctx.fec_encode_packets_device(h, src, 1, 17, out=out)
        path = ctx.fec_sender_info()["path"]
        ctx.synchronize()
        assert must_be is None or path == must_be, (shift, path)
        host = big.cpu().numpy()
        assert (host[:start] == 0xA5).all() and (host[start + nbytes:] == 0xA5).all(), f"guard band touched at shift {shift} ({path})"
        assert np.array_equal(host[start:start + nbytes].reshape(F * code.n, 8 + S), want), (shift, path)


# ------------------------------------------------------------------------------------------ 4. the header comment's contract
@pytest.mark.parametrize("which,S,F", [(1, 1024, 9), (1, 128, 9), (1, 16, 9), (1, 1, 9), (3, 1024, 5), (0, 256, 9), ("heavy", 128, 9)])
def test_same_bytes_as_encode_then_packetize(ctx, which, S, F):
    h, code = get_code(ctx, which)
    src = make_source(F, code.k, S, seed=60 + S)
    got = send(ctx, h, src, 0xAB, 252)
    cw = ctx.encode(h, src[:, :, 0].contiguous() if S == 1 else src)
    want = ctx.fec_packetize_device(cw.view(F, code.n, S), 0xAB, 252)
    ctx.synchronize()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------ 5. FecTxDevice
def test_fec_tx_device_numbers_blocks_across_calls(ctx):
    h, code = get_code(ctx, 1)
    S = 128
    src = make_source(260, code.k, S, seed=70)
    tx = ctx.fec_tx_device(h, S)
    assert tx.next_block == 0
    parts = [tx.send(src[a:b]) for a, b in ((0, 100), (100, 200), (200, 260))]
    assert tx.next_block == 4                                     # 260 mod 256
    whole = ctx.fec_encode_packets_device(h, src, 1, 0)
    ctx.synchronize()
    assert torch.equal(torch.cat(parts), whole)


# ------------------------------------------------------------------------------------------ 6. end to end on the device
def test_end_to_end_fused_sender_to_decode_frames(ctx):
    from test_gpu_wire_device import channel
    h, code = get_code(ctx, 1)
    n, k, S, F = code.n, code.k, 1024, 260
    src = make_source(F, k, S, seed=21)
    tx = ctx.fec_tx_device(h, S)
    pk = tx.send(src)
    assert ctx.fec_sender_info()["path"] == "fused"
    pk = channel(pk, n, seed=22, loss=(0.1,), window=300, dup=0.01, dup_flip=False, bad_sym=0.0, foreign=0.0)
    rx = ctx.fec_rx_device(n, k, S)
    blocks, results = [], []
    pos = 0
    while pos < pk.shape[0]:
        b, sym, er, used = rx.push_many(pk[pos:], 64)
        pos += used
        if len(b):
            results.append(ctx.decode_frames(h, sym, er))
            blocks += [int(x) for x in b]
    while True:
        r = rx.flush()
        if r is None:
            break
        results.append(ctx.decode_frames(h, r[1][None].contiguous(), r[2][None].contiguous()))
        blocks.append(int(r[0]))
    rx.close()
    ctx.synchronize()
    assert blocks == [i & 0xFF for i in range(F)]                 # every block closes, in order
    src_h = src.cpu().numpy()
    i = good = 0
    for res in results:
        out, st, rs = res.out.cpu().numpy(), res.status.cpu().numpy(), res.residual_src.cpu().numpy()
        for f in range(out.shape[0]):
            if st[f] in (api.ST_MP_DONE, api.ST_ML_SOLVED):
                assert np.array_equal(out[f, :k], src_h[i]), f"block {i}: decodable but not the transmitted source"
                assert rs[f] == 0
                good += 1
            i += 1
    assert i == F and good >= F // 2


# ------------------------------------------------------------------------------------------ 7. argument errors
def test_sender_argument_errors(ctx):
    L = api.load_library()
    h, code = get_code(ctx, 1)
    n, k, S, F = code.n, code.k, 16, 2
    src_d = make_source(F, k, S, seed=80)
    pk_d = torch.full((F * n, 8 + S), 0x5A, dtype=torch.uint8, device="cuda")
    src_h = np.zeros((F, k, S), dtype=np.uint8)
    pk_h = np.zeros((F * n, 8 + S), dtype=np.uint8)
    good = ctx.fec_encode_packets_device(h, src_d, 1, 0).clone()
    ctx.synchronize()

    def refused(rc, want, text=None):
        assert rc == want
        msg = L.ldpc_amd_last_error(ctx._h)
        assert msg and (text is None or text in msg), msg
        # the context is still usable: a correct call succeeds and gives the right bytes
        again = ctx.fec_encode_packets_device(h, src_d, 1, 0)
        ctx.synchronize()
        assert torch.equal(again, good)

    call = L.ldpc_amd_fec_encode_packets_dev
    refused(call(ctx._h, h, S, F, src_h.ctypes.data, 1, 0, pk_d.data_ptr()), EINVAL, b"device pointers")
    refused(call(ctx._h, h, S, F, src_d.data_ptr(), 1, 0, pk_h.ctypes.data), EINVAL, b"device pointers")
    pinned = torch.zeros((F * n, 8 + S), dtype=torch.uint8).pin_memory()
    refused(call(ctx._h, h, S, F, src_d.data_ptr(), 1, 0, pinned.data_ptr()), EINVAL, b"device pointers")
    src24 = torch.zeros((F, k, 24), dtype=torch.uint8, device="cuda")
    pk24 = torch.zeros((F * n, 8 + 24), dtype=torch.uint8, device="cuda")
    refused(call(ctx._h, h, 24, F, src24.data_ptr(), 1, 0, pk24.data_ptr()), EUNSUP, b"multiple of 16")
    nt = non_triangular_code()
    hnt = ctx.register_code(nt)
    src_nt = torch.zeros((F, nt.k, S), dtype=torch.uint8, device="cuda")
    pk_nt = torch.zeros((F * nt.n, 8 + S), dtype=torch.uint8, device="cuda")
    refused(call(ctx._h, hnt, S, F, src_nt.data_ptr(), 1, 0, pk_nt.data_ptr()), EUNSUP, b"triangle form")
    refused(call(ctx._h, 999, S, F, src_d.data_ptr(), 1, 0, pk_d.data_ptr()), ENOCODE, b"unknown code handle")
    refused(call(ctx._h, h, S, -1, src_d.data_ptr(), 1, 0, pk_d.data_ptr()), EINVAL)
    # overlapping buffers: the packets start inside the source, and the source inside the packets
    both = torch.zeros(F * k * S + F * n * (8 + S), dtype=torch.uint8, device="cuda")
    refused(call(ctx._h, h, S, F, both.data_ptr(), 1, 0, both.data_ptr() + F * k * S - 16), EINVAL, b"overlap")
    refused(call(ctx._h, h, S, F, both.data_ptr() + 64, 1, 0, both.data_ptr()), EINVAL, b"overlap")
    # nframes = 0: OK, and nothing is touched (not even looked at: null pointers pass)
    pk_d.fill_(0x5A)
    assert call(ctx._h, h, S, 0, src_d.data_ptr(), 1, 0, pk_d.data_ptr()) == 0
    assert call(ctx._h, h, S, 0, None, 1, 0, None) == 0
    ctx.synchronize()
    assert bool((pk_d == 0x5A).all())
