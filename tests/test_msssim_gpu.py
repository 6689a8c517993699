"""MS-SSIM / SSIM on the GPU: the HIP kernels of csrc/msssim.hip against the fp64 torch-op restatement of
pytorch_msssim's ms_ssim (tests/msssim_ref.py, bound from the restatement's own fp32 error) and against the host twin;
bit-reproducibility, batch independence, graph capture; CompressionMetrics on the model's output and the inference
CLI's ms_ssim column."""
import csv
import re

import numpy as np
import pytest
import torch

import msssim_ref as R
from helpers import build_model

pytestmark = pytest.mark.gpu

CASES = [(s, d) for s in R.SHAPES for d in R.DISTORTIONS]
IDS = [f"{'x'.join(map(str, s))}-{d}" for s, d in CASES]


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape,dist", CASES, ids=IDS)
def test_device_matches_restatement_and_host_twin(shape, dist):
    from hyres_hip import metrics
    ref = R.case(shape, dist)
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    out, raw = metrics.per_level(x, y)
    assert out.is_cuda and raw.is_cuda and out.dtype == torch.float32
    R.check(out, raw, ref, f"device {shape} {dist}")
    out_h, raw_h = metrics.per_level(ref["x"], ref["y"])
    assert ((out.cpu().double() - out_h.double()).abs() <= ref["tol_out"]).all()
    assert ((raw.cpu().double() - raw_h.double()).abs() <= ref["tol_raw"]).all()
    if dist == "same":
        assert torch.equal(out.cpu(), torch.ones(shape[0]))
    if dist == "inverted":
        assert (ref["raw"][0] < 0).all() and (raw[0] < 0).all() and torch.equal(out.cpu(), torch.zeros(shape[0]))
    # two calls on the same input: the same bits
    out2, raw2 = metrics.per_level(x, y)
    assert torch.equal(out, out2) and torch.equal(raw, raw2)
    got = metrics.ms_ssim(x, y)
    assert got.is_cuda and got.dim() == 0
    assert abs(float(got) - float(ref["out"].mean())) <= float(ref["tol_out"].max())


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_batch_equals_images_run_singly(shape):
    """A reduction that ran across planes or depended on the grid's z extent would show here."""
    from hyres_hip import metrics
    ref = R.case(shape, "noise")
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    out, raw = metrics.per_level(x, y)
    for b in range(shape[0]):
        o1, r1 = metrics.per_level(x[b:b + 1], y[b:b + 1])
        assert torch.equal(o1[0], out[b]) and torch.equal(r1[:, 0], raw[:, b])


def test_ssim_on_device():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[1], "blur")
    want = R.ssim_ref(ref["x"], ref["y"])
    d = (R.ssim_ref(ref["x"], ref["y"], torch.float32).double() - want).abs().max()
    got = metrics.ssim(ref["x"].to(dev()), ref["y"].to(dev()), size_average=False)
    assert got.is_cuda and ((got.cpu().double() - want).abs() <= R.bound(d)).all()


def test_noncontiguous_inputs_give_the_contiguous_result():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[2], "noise")
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    want = metrics.ms_ssim(x, y, size_average=False)
    xcl = x.contiguous(memory_format=torch.channels_last)
    wide = torch.zeros(1, 3, 180, 216, device=dev())
    wide[:, :, 2:178, 5:213] = y
    ysl = wide[:, :, 2:178, 5:213]
    assert not xcl.is_contiguous() and not ysl.is_contiguous()
    assert torch.equal(metrics.ms_ssim(xcl, ysl, size_average=False), want)


def test_ms_ssim_is_capture_legal():
    """Captured once and replayed on a second pair, then on the first again: each replay gives that pair's eager bits
    (no sync, no allocation outside the graph's pool, no host read, nothing left over from the previous replay)."""
    from hyres_hip import metrics
    D = dev()
    shape = R.SHAPES[0]
    a, b = R.case(shape, "noise"), R.case(shape, "blur")
    pairs = [(a["x"].to(D), a["y"].to(D)), (b["x"].to(D), b["y"].to(D))]
    eager = [(metrics.ms_ssim(x, y).clone(), metrics.ms_ssim(x, y, size_average=False).clone()) for x, y in pairs]
    assert not torch.equal(eager[0][1], eager[1][1])
    sx, sy = pairs[0][0].clone(), pairs[0][1].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.ms_ssim(sx, sy)  # warm-up: this stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        per_image = metrics.ms_ssim(sx, sy, size_average=False)
        avg = per_image.mean()
    for k in (1, 0):
        sx.copy_(pairs[k][0])
        sy.copy_(pairs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(per_image, eager[k][1]) and torch.equal(avg, eager[k][0]), k
        assert ((per_image.cpu().double() - (a, b)[k]["out"]).abs() <= (a, b)[k]["tol_out"]).all()


def _png(path, x):
    from PIL import Image
    Image.fromarray((x[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(path)


@pytest.fixture(scope="module")
def model():
    net, _ = build_model()
    net = net.to(dev()).eval()
    assert net.update(force=True)
    return net


def test_compression_metrics_on_the_model_output(model):
    """CompressionMetrics.msssim(x, decompress(compress(x))["x_hat"]) at 1x3x192x224 against the restatement on the
    same two tensors."""
    from src.utils import CompressionMetrics
    x = R.smooth_field((1, 3, 192, 224), 11).to(dev())
    with torch.no_grad():
        x_hat = model.decompress(model.compress(x))["x_hat"]
    assert x_hat.shape == x.shape
    got = CompressionMetrics(device=dev()).msssim(x, x_hat)
    want, _ = R.ms_ssim_ref(x.cpu(), x_hat.cpu(), torch.float64)
    d = (R.ms_ssim_ref(x.cpu(), x_hat.cpu(), torch.float32)[0].double() - want).abs().max()
    print(f"model 192x224: ms-ssim {got:.6f} ref {float(want):.6f} d {float(d):.3e} err {abs(got - float(want)):.3e}")
    assert isinstance(got, float) and 0 < got <= 1
    assert abs(got - float(want)) <= float(R.bound(d))


def _run_cli(tmp_path, x, capsys):
    from src.inference import main as infer_main
    ck = tmp_path / "ckpt.pth.tar"
    torch.save({"state_dict": {k: v.cpu() for k, v in build_model()[0].state_dict().items()}}, ck)
    _png(tmp_path / "img.png", x)
    out = tmp_path / "out"
    infer_main(["--checkpoint", str(ck), "--input", str(tmp_path / "img.png"), "--output", str(out),
                "--jpeg-quality", "50"])
    rows = list(csv.DictReader(open(out / "metrics.csv")))
    assert len(rows) == 1
    return rows[0], capsys.readouterr().out


def test_inference_cli_reports_ms_ssim(tmp_path, capsys):
    row, text = _run_cli(tmp_path, R.smooth_field((1, 3, 192, 224), 12), capsys)
    v = float(row["ms_ssim"])
    assert 0 < v <= 1
    per_image = re.findall(r"PSNR: [-\d.]+ dB, MS-SSIM: ([\d.]+)", text)
    average = re.findall(r"^MS-SSIM: ([\d.]+)$", text.split("Average metrics:")[1], flags=re.M)
    assert per_image == [f"{v:.4f}"] and average == [f"{v:.4f}"], text


def test_inference_cli_keeps_zero_below_the_minimum_size(tmp_path, capsys):
    row, text = _run_cli(tmp_path, R.smooth_field((1, 3, 64, 64), 13), capsys)
    assert float(row["ms_ssim"]) == 0.0 and "MS-SSIM: 0.0000" in text
