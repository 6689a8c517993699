"""Images of any size on the GPU: the any-size device JPEG codec and decoder (``any_size=True``) against Pillow's
libjpeg-turbo (tests/golden/jpeg_ragged_cases.npz) and the host twin, ``hyres_pad2d`` against F.pad / slicing, and
the model on images whose sides are not multiples of 32 (the residual is padded, the JPEG is not).
"""
import io
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

from helpers import build_model
from test_jpeg_ragged_cpu import CASES, as_input, case_named, corrupt_files, want_of

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 40, 56), (1, 3, 33, 47)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def noise(shape, seed):
    imgs = [torch.randint(0, 256, shape[1:], generator=torch.Generator().manual_seed(seed + i)) for i in range(shape[0])]
    return torch.stack(imgs).float() / 255.0


def by_shape():
    out = defaultdict(list)
    for c in CASES:
        out[c["u8"].shape[:2]].append(c)
    return out


# ---------------------------------------------------------------------------------------------- JPEG codec
def test_device_codec_equals_pillow_and_the_host_twin():
    """Every fixture case, batched by size and quality: files, sizes and pixels."""
    from hyres_hip import jpeg_device
    n = 0
    for cs in by_shape().values():
        for q in sorted({c["quality"] for c in cs}):
            cq = [c for c in cs if c["quality"] == q]
            x = torch.cat([as_input(c["u8"]) for c in cq])
            dec, files = jpeg_device.encode(x.to(dev()), q, any_size=True)
            dec_r, sizes = jpeg_device.roundtrip(x.to(dev()), q, any_size=True)  # the sizes-only path
            dec_h, files_h = jpeg_device.encode_host(x, q, any_size=True)
            assert files == [c["file"] for c in cq] and files == files_h, (cq[0]["name"], q)
            assert sizes.tolist() == [len(c["file"]) for c in cq]
            assert torch.equal(dec.cpu(), torch.cat([want_of(c) for c in cq])), (cq[0]["name"], q)
            assert torch.equal(dec.cpu(), dec_h) and torch.equal(dec_r, dec)
            n += len(cq)
    assert n == len(CASES)


@pytest.mark.parametrize("sub_bits", (32, 0))
def test_fixture_files_decode_on_the_device(sub_bits):
    from hyres_hip import jpeg_device
    for cs in by_shape().values():
        files = [c["file"] for c in cs]
        dec, status, rounds = jpeg_device.decode_tensors(jpeg_device.stage(files, dev(), any_size=True), sub_bits)
        dec_h, rounds_h = jpeg_device.decode_host(files, sub_bits, return_rounds=True, any_size=True)
        assert status.cpu().tolist() == [0] * len(cs)
        assert torch.equal(dec.cpu(), torch.cat([want_of(c) for c in cs])), cs[0]["name"]
        assert torch.equal(dec.cpu(), dec_h) and torch.equal(rounds.cpu(), rounds_h)
    f = [case_named("noise_13x21_q50")["file"]]
    assert torch.equal(jpeg_device.decode(f, dev(), sub_bits, any_size=True).cpu(), want_of(case_named("noise_13x21_q50")))
    with pytest.raises(ValueError):
        jpeg_device.decode(f, dev(), sub_bits)  # the strict entry point keeps refusing the file


@pytest.mark.parametrize("name", ["truncated", "zeroed_tail", "planted_rst"])
def test_corrupt_ragged_files_on_the_device(name):
    from hyres_hip import jpeg_device
    f = corrupt_files()[name]
    _, status_h = jpeg_device.decode_host([f], check=False, any_size=True)
    _, status = jpeg_device.decode([f], dev(), check=False, any_size=True)
    assert status.cpu().tolist() == status_h.tolist() and int(status_h[0]) != 0
    good = case_named("noise_33x47_q50")
    assert torch.equal(jpeg_device.decode([good["file"]], dev(), any_size=True).cpu(), want_of(good))


def test_roundtrip_any_is_capture_legal():
    """hyres_jpeg_roundtrip_any at 13 x 21 captured once and replayed on new input gives the eager result."""
    from hyres_hip import jpeg_device
    D = dev()
    x1, x2 = noise((2, 3, 13, 21), 11).to(D), noise((2, 3, 13, 21), 23).to(D)
    static = x1.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        jpeg_device.roundtrip(static, 50, any_size=True)  # warm-up: the stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        dec, sizes = jpeg_device.roundtrip(static, 50, any_size=True)
    for x in (x2, x1):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        dec_h, sizes_h = jpeg_device.roundtrip_host(x.cpu(), 50, any_size=True)
        assert torch.equal(dec.cpu(), dec_h) and torch.equal(sizes.cpu(), sizes_h)


# ---------------------------------------------------------------------------------------------- pad2d
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
@pytest.mark.parametrize("src,dst", [((2, 40, 56, 3), (64, 64)), ((1, 33, 47, 192), (64, 64))])
def test_pad2d_equals_pad_and_slicing(src, dst, dtype):
    from hyres_hip import _lib as L
    D = dev()
    B, H, W, C = src
    Hp, Wp = dst
    g = torch.Generator().manual_seed(5)
    x = torch.randn(src, generator=g).to(dtype).to(D)
    big = torch.randn((B, Hp, Wp, C), generator=g).to(dtype).to(D)
    io = L.dt_mask(x, x, L.IO_X16, L.IO_Y16)

    def run(a, Hs, Ws, out, Hd, Wd, acc):
        L.call("hyres_pad2d", a.data_ptr(), a.stride(2), Hs, Ws, out.data_ptr(), out.stride(2), Hd, Wd, B, C, acc, io,
               L.stream())
        torch.cuda.synchronize()
        return out

    pad = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
    assert torch.equal(run(x, H, W, torch.full_like(big, float("nan")), Hp, Wp, 0), pad)
    assert torch.equal(run(big, Hp, Wp, torch.full_like(x, float("nan")), H, W, 0), big[:, :H, :W])
    # gradient fan-in: fp32 adds rounded once to the storage type, as a torch add of the same operands is
    assert torch.equal(run(x, H, W, big.clone(), Hp, Wp, 1), (big.float() + pad.float()).to(dtype))
    assert torch.equal(run(big, Hp, Wp, x.clone(), H, W, 1), (x.float() + big[:, :H, :W].float()).to(dtype))
    # a channel slice of a wider buffer on either side (pixel stride > C)
    wide = torch.randn((B, Hp, Wp, C + 5), generator=g).to(dtype).to(D)
    got = run(x, H, W, wide.clone()[..., 2:2 + C], Hp, Wp, 0)
    assert got.stride(2) == C + 5 and torch.equal(got, pad)
    assert torch.equal(run(wide[..., 1:1 + C], Hp, Wp, torch.empty_like(x), H, W, 0), wide[:, :H, :W, 1:1 + C])


# ---------------------------------------------------------------------------------------------- model
def eval_model(**coder):
    net, _ = build_model()
    if coder:
        from models import LightWeightCheckerboard, ResidualJPEGCompression
        from hyres_hip.weights import synthetic_state_dict
        net = ResidualJPEGCompression(base_model=LightWeightCheckerboard(**coder), jpeg_quality=50)
        torch.nn.Module.load_state_dict(net, synthetic_state_dict(net.state_dict()), strict=True)
    net = net.to(dev()).eval()
    assert net.update(force=True)
    return net


@pytest.fixture(scope="module")
def net_eval():
    return eval_model()


@pytest.mark.parametrize("shape", SHAPES)
def test_model_forward_pads_the_residual_only(net_eval, shape):
    net = net_eval
    B, _, H, W = shape
    x = noise(shape, 3).to(dev())
    with torch.no_grad():
        out = net(x)
        for k in ("x_hat", "jpeg_decoded", "residual", "residual_hat"):
            assert tuple(out[k].shape) == shape, k
        assert tuple(out["likelihoods"]["y"].shape) == (B, 192, 8, 8)
        assert tuple(out["likelihoods"]["z"].shape) == (B, 128, 2, 2)
        assert torch.equal(out["residual"], x - out["jpeg_decoded"])
        padded = F.pad(out["residual"], (0, 64 - W, 0, 64 - H))
        want = net.residual_model(padded)
        assert torch.equal(out["residual_hat"], want["x_hat"][..., :H, :W])
        assert torch.equal(out["likelihoods"]["y"], want["likelihoods"]["y"])
        # the JPEG stage saw the true image: Pillow's round trip of the H x W bytes
        d_host, _ = net.jpeg(x.cpu())
        assert torch.equal(out["jpeg_decoded"].cpu(), d_host)
        # an aligned input records no pad op and launches no kernel for it
        from hyres_hip import refine_ops as R
        calls = []
        real = R.pad2d
        R.pad2d = lambda *a, **k: calls.append(a) or real(*a, **k)
        try:
            net(noise((1, 3, 64, 96), 9).to(dev()))
            assert not calls
            net(x)
            assert len(calls) == 2
        finally:
            R.pad2d = real


def test_refine_runs_at_the_true_size():
    """MultiScaleRefine at 33 x 47 (its 1/2 and 1/4 scales are 16 x 23 and 8 x 11, as F.interpolate's floor gives)
    against the oracle's refine, to the 1e-4 the eval fixtures are held to."""
    from helpers import oracle_from, rel_err
    net, sd = build_model()
    net = net.to(dev()).eval()
    x0 = noise((1, 3, 33, 47), 21)
    with torch.no_grad():
        got = net.refine(x0.to(dev()))
        want = oracle_from(sd)[0].refine(x0)
    assert tuple(got.shape) == (1, 3, 33, 47)
    assert rel_err(got.cpu(), want) < 1e-4


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_compress_decompress_roundtrip_at_any_size(net_eval, shape, amp):
    """The criterion of test_parity_gpu.test_compress_decompress_roundtrip: the decoded residual equals the eval
    forward's residual_hat (clamped) and x_hat the reference formula on it, both to 1e-6."""
    from hyres_hip import ops as O
    net = net_eval
    B, _, H, W = shape
    x = noise(shape, 5).to(dev())
    ctx = torch.autocast("cuda", dtype=torch.float16) if amp else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        fwd = net(x)
        c = net.compress(x)
        d = net.decompress(c)
        dres = net.residual_model.decompress(c["strings"], c["shape"])["x_hat"][..., :H, :W]
        x0 = fwd["jpeg_decoded"] + dres
        with O.f16_region():
            want = torch.clamp(x0 + net.refine(x0), 0, 1)
    assert tuple(c["shape"]) == (2, 2) and len(c["jpeg_buffers"]) == B
    assert tuple(d["x_hat"].shape) == shape
    assert float((dres - fwd["residual_hat"].clamp(0, 1)).abs().max()) <= 1e-6
    assert float((d["x_hat"] - want).abs().max()) <= 1e-6
    from PIL import Image
    assert Image.open(io.BytesIO(c["jpeg_buffers"][0].getvalue())).size == (W, H)  # a real JPEG of the real image


@pytest.mark.parametrize("coder", [{}, {"device_coder": True, "coder_segment_rows": 0},
                                   {"device_coder": True, "coder_segment_rows": 512}], ids=["host", "hrw1", "hrw2"])
def test_model_with_the_any_size_device_codec_equals_the_host_codec(coder, monkeypatch):
    net = eval_model(**coder)
    for shape in SHAPES:
        x = noise(shape, 7).to(dev())
        out, comp, dcmp = {}, {}, {}
        with torch.no_grad():
            net.jpeg.device_codec, net.jpeg.any_size = False, False
            out[0], comp[0] = net(x), net.compress(x)
            dcmp[0] = net.decompress(comp[0])
            net.jpeg.device_codec = True
            assert not net.jpeg.on_device(x)  # the first opt-in alone keeps the host path
            net.jpeg.any_size = True
            assert net.jpeg.on_device(x)
            with monkeypatch.context() as m:
                def pillow(*a, **k):
                    raise AssertionError("the device path must not call Pillow")
                m.setattr(net.jpeg.jpeg, "decode", pillow)
                m.setattr(net.jpeg.jpeg, "encode", pillow)
                out[1], comp[1] = net(x), net.compress(x)
                dcmp[1] = net.decompress(comp[1])
                assert torch.equal(net.decompress(comp[0])["x_hat"], dcmp[0]["x_hat"])  # the host codec's buffers
        assert out[1]["jpeg_bpp_loss"].is_cuda
        assert out[1]["jpeg_bpp_loss"].cpu().numpy() == out[0]["jpeg_bpp_loss"].cpu().numpy()
        for k in ("x_hat", "jpeg_decoded", "residual", "residual_hat"):
            assert torch.equal(out[1][k], out[0][k]), k
        assert [b.getvalue() for b in comp[1]["jpeg_buffers"]] == [b.getvalue() for b in comp[0]["jpeg_buffers"]]
        assert comp[1]["strings"] == comp[0]["strings"] and comp[1]["shape"] == comp[0]["shape"]
        assert torch.equal(dcmp[1]["x_hat"], dcmp[0]["x_hat"]) and tuple(dcmp[1]["x_hat"].shape) == shape


def test_train_step_at_a_ragged_size_matches_the_oracle(monkeypatch):
    """One train-mode forward + backward at 2 x 3 x 40 x 56 against the same composition in torch autograd around the
    oracle's sub-modules (pad -> residual model -> crop -> refine), decision-exact, with the tolerances
    test_parity_gpu.py allows the aligned train-step fixtures: the loss within TOL, every parameter gradient
    normwise within 1e-3."""
    import oracle
    from test_parity_gpu import TOL, _check_grads, _hip_model, _hip_train_step, _nhwc_noise, _oracle_following
    shape = SHAPES[0]
    B, _, H, W = shape

    def forward(self, x, jpeg_decoded, jpeg_bpp=0.0, training=False, noisequant=False, noise=None, trace=None):
        T = {}
        residual = x - jpeg_decoded
        res = self.codec_forward(F.pad(residual, (0, 64 - W, 0, 64 - H)), training, noisequant, noise, T)
        residual_hat = res["x_hat"][..., :H, :W]
        x0 = jpeg_decoded + residual_hat
        x_hat = torch.clamp(x0 + self.refine(x0, T), 0, 1)
        return {"x_hat": x_hat, "likelihoods": res["likelihoods"], "jpeg_bpp_loss": torch.tensor(jpeg_bpp),
                "jpeg_decoded": jpeg_decoded, "residual": residual, "residual_hat": residual_hat}

    monkeypatch.setattr(oracle.Oracle, "forward", forward)
    net, _ = _hip_model()
    net.train()
    x = noise(shape, 13)
    jpeg, jb = net.jpeg(x)
    jb = float(jb)
    ng = torch.Generator().manual_seed(45)
    nz = {"z": torch.rand((B, 128, 2, 2), generator=ng) - 0.5, "y": torch.rand((B, 192, 8, 8), generator=ng) - 0.5}
    out, crit, dec, hats = _hip_train_step(net, x, jpeg, jb, False, _nhwc_noise(nz, {"z": "z", "y": "y"}, dev()), 0.045)
    assert tuple(out["x_hat"].shape) == shape and tuple(out["residual_hat"].shape) == shape
    torch.set_num_threads(16)
    ref, terms, loss64, followed = _oracle_following({"x": x, "jpeg_decoded": jpeg}, jb, False, nz, 0.045, dec, hats)
    print(f"loss hip {float(crit['loss']):.6f} oracle {loss64:.6f}; followed {followed}")
    assert abs(float(crit["loss"]) - loss64) <= TOL * abs(loss64), (float(crit["loss"]), loss64)
    rows = _check_grads(net, ref, terms)
    print("worst grads", [f"{e:.2e} {k}" for e, k in rows[:5]])


def test_inference_cli_on_a_ragged_png(tmp_path):
    import csv
    import numpy as np
    from PIL import Image
    from src.inference import main as infer_main
    net, _ = build_model()
    ck = tmp_path / "ckpt.pth.tar"
    torch.save({"state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, ck)
    img = (noise((1, 3, 40, 56), 17)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "img.png")
    out = tmp_path / "out"
    infer_main(["--checkpoint", str(ck), "--input", str(tmp_path / "img.png"), "--output", str(out),
                "--jpeg-quality", "50"])
    rows = list(csv.DictReader(open(out / "metrics.csv")))
    assert len(rows) == 1 and rows[0]["filename"] == "img.png"
    r = rows[0]
    assert float(r["y_bpp"]) > 0 and float(r["z_bpp"]) > 0 and float(r["jpeg_bpp"]) > 0
    assert abs(float(r["total_bpp"]) - (float(r["jpeg_bpp"]) + float(r["y_bpp"]) + float(r["z_bpp"]))) < 1e-9
    assert Image.open(out / "img_recon.png").size == (56, 40)
