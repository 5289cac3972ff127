"""GPU test of the chunk loop of the receivers' decode driver (csrc/rx_host.h): the composed form of a decode call gathers at most
256 MiB of received symbols at a time, so a second chunk exists only when one call closes more than 256 MiB worth of blocks.  No other
test reaches that; this one does, at the smallest size that can, through the windowed single-flow receiver, whose info record counts
the launch_decode calls."""
import pytest

from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S, W, A = 1024, 4, 10
NEED_FREE = 4 << 30   # the test holds about 1.5 GB of device memory


def test_composed_decode_in_two_chunks():
    """The built-in (2000, 1000) code with S = 1024: a frame is 2 048 000 bytes, so a chunk is floor(256 MiB / frame) = 131 slots.
    131 + W + 2 frames in ONE decode_many call close at least 132 blocks: two chunks, two launch_decode calls.  The reference is a second
    receiver's push_many + Context.decode_frames, which has no chunk loop; everything is compared on the device."""
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"torch.cuda.mem_get_info() reports {free} bytes free, under the 4 GiB this test asks for")
    code = codes.load_builtin(0)
    n, k = code.n, code.k
    frame = n * S
    chunk = (256 << 20) // frame
    assert (n, k, chunk) == (2000, 1000, 131)
    F = chunk + W + 2
    with api.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        h = ctx.load_builtin_code(0, codes.DEFAULT_COEF_SEED[0])
        src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(77))
        sent = ctx.fec_encode_packets_device(h, src, 1, 0)
        assert ctx.fec_sender_info()["path"] == "fused"
        keep = torch.arange(sent.shape[0], device="cuda") % 10 != 9   # every tenth packet is lost
        pk = sent[keep].contiguous()
        del src, sent
        ctx.configure("LDPC_AMD_RX_PKT", 0)
        try:
            with ctx.fec_rx_window(n, k, S, W, A) as rx:
                b, fr, used = rx.decode_many(h, pk, F)
            info = ctx.fec_rx_window_info()
        finally:
            ctx.configure("LDPC_AMD_RX_PKT", None)
        print("closed", len(b), "consumed", used, "of", pk.shape[0], info)
        assert len(b) >= chunk + 1 and used == pk.shape[0]
        assert info["path"] == "composed" and info["blocks"] == len(b) and info["launches"] == 2
        assert info["scratch_bytes"] == chunk * frame <= 256 << 20
        with ctx.fec_rx_window(n, k, S, W, A) as rx:
            ref_b, sym, er, ref_used = rx.push_many(pk, F)
        ref = ctx.decode_frames(h, sym, er)
        assert ref_used == used and torch.equal(torch.from_numpy(b.copy()), torch.from_numpy(ref_b.copy()))
        for name, got, want in zip(api.DecodedFrames._fields, fr, ref):
            assert got.is_cuda and want.is_cuda and got.shape == want.shape and torch.equal(got, want), name
        assert int((ref.status <= 1).sum()) == len(b), "every block decodes at this loss"
        torch.cuda.synchronize()
