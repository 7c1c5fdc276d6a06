"""The opt-in bf16 inference path without a GPU: the C ABI of csrc/sconv_bf16.hip is declared, bound and exported, the
eligibility rule, the command-line flags, the `precision` arguments' validation, and the rounding helper the GPU tests
(tests/test_gpu_bf16.py) build their float64 reference with."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_SYMBOLS = ("lidog_pack_kernels_bf16", "lidog_sconv_gemm_bf16", "lidog_sconv_os_bn_bf16")


def test_bf16_symbols_are_declared_bound_and_exported():
    from lidog_amd import _lib, build
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in BF16_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "sconv_bf16.hip" in build.SOURCES
    # arguments + the stream every `call` appends
    assert len(_lib.SIGNATURES["lidog_pack_kernels_bf16"]) == 6
    assert len(_lib.SIGNATURES["lidog_sconv_gemm_bf16"]) == 13
    assert len(_lib.SIGNATURES["lidog_sconv_os_bn_bf16"]) == len(_lib.SIGNATURES["lidog_sconv_os_bn"])


@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34IBN"])
def test_eligible_excludes_exactly_the_stem_and_the_classifier(kind):
    import lidog_amd
    import lidog_amd.me as ME
    from lidog_amd import precision
    torch.manual_seed(0)
    model = getattr(lidog_amd, kind)(in_channels=1, out_channels=7, D=3)
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, ME._ConvBase)]
    assert len(convs) > 40
    out = sorted(n for n, m in convs if not precision.eligible(m))
    assert out == ["conv0p1s1", "final"]
    assert (model.conv0p1s1.in_channels, model.final.out_channels) == (1, 7)
    for n, m in convs:
        assert precision.eligible(m) == (m.in_channels % 32 == 0 and m.out_channels % 32 == 0), n
    # not a convolution, and odd channel counts on either side
    assert not precision.eligible(model.bn0) and not precision.eligible(torch.nn.Linear(32, 32))
    for cin, cout, ok in ((32, 32, True), (96, 128, True), (48, 32, False), (32, 48, False), (16, 16, False)):
        assert precision.eligible(ME.MinkowskiConvolution(cin, cout, kernel_size=3, dimension=3)) == ok
    assert precision.eligible(ME.MinkowskiConvolutionTranspose(64, 32, kernel_size=2, stride=2, dimension=3))


def test_cli_flags():
    from lidog_amd.eval_target import parse_args as eval_args
    from lidog_amd.train import parse_args as train_args, val_precision_of
    assert eval_args(["--checkpoint", "c.ckpt"]).precision == "fp32"
    assert eval_args(["--checkpoint", "c.ckpt", "--precision", "bf16"]).precision == "bf16"
    assert eval_args(["--checkpoint", "c.ckpt", "--precision", "fp32"]).precision == "fp32"
    assert val_precision_of(train_args([])) == "fp32"
    assert val_precision_of(train_args(["--val-precision", "bf16"])) == "bf16"
    assert val_precision_of(train_args(["--val-precision", "fp32", "--val-scans", "4"])) == "fp32"
    for parse, argv in ((eval_args, ["--checkpoint", "c.ckpt", "--precision", "fp16"]), (train_args, ["--val-precision", "fp16"]),
                        (train_args, ["--val-precision"])):
        with pytest.raises(SystemExit) as e:
            parse(argv)
        assert e.value.code == 2


def _cpu_model():
    import lidog_amd
    torch.manual_seed(0)
    return lidog_amd.MinkUNet34(in_channels=1, out_channels=7, D=3)


def test_an_unknown_precision_is_a_value_error_before_anything_runs(monkeypatch):
    from lidog_amd import _lib, evaluate, precision
    from lidog_amd.train import Fit

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    for mod in (_lib, precision, evaluate.ME):
        monkeypatch.setattr(mod, "call", no_launch)
    model = _cpu_model()
    coords, feats = torch.zeros((4, 4), dtype=torch.int32), torch.ones((4, 1))
    for bad in ("fp16", "BF16", 16, ""):
        with pytest.raises(ValueError, match="precision"):
            precision.resolve(bad)
        with pytest.raises(ValueError, match="precision"):
            evaluate.predict(model, coords, feats, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            evaluate.Predictor(model, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            evaluate.evaluate(model, [], precision=bad)
        with pytest.raises(ValueError, match="precision"):
            evaluate.TargetEvaluator(model, precision=bad)
    with pytest.raises(ValueError, match="precision"):
        Fit(val_precision="fp16", device="cpu")
    assert (precision.resolve(None), precision.resolve("fp32"), precision.resolve("bf16")) == (None, False, True)
    assert model.training                      # predict() refused before it touched the model


def test_bf16_on_a_cpu_model_raises_through_require_gpu():
    from lidog_amd import evaluate, precision
    model = _cpu_model()
    coords, feats = torch.zeros((4, 4), dtype=torch.int32), torch.ones((4, 1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        precision.Bf16Kernels(model)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        with precision.bf16_inference(model):
            pass
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        evaluate.predict(model, coords, feats, precision="bf16")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        evaluate.Predictor(model, precision="bf16")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        evaluate.TargetEvaluator(model, precision="bf16").run(iter([({"coords_int": coords}, [0])]), 1)
    assert precision.current() is None


def test_contexts_nest_and_restore():
    from lidog_amd import precision

    class Table:
        def get(self, conv):
            return None
    assert precision.current() is None
    with precision.bf16_inference(None, Table()) as outer:
        assert precision.current() is outer and isinstance(outer, precision.Bf16Context)
        with precision.scope(None, None) as same:
            assert same is outer and precision.current() is outer           # None changes nothing
        with precision.scope(None, "fp32"):
            assert precision.current() is None
            with precision.scope(None, "bf16", Table()) as inner:
                assert precision.current() is inner and inner is not outer
            assert precision.current() is None
        assert precision.current() is outer
        outer.count("conv", precision.FP32)
        outer.count("conv", precision.OS_BN)
        assert outer.launches == {precision.FP32: 1, precision.OS_BN: 1}
        assert outer.routes == {"conv": {precision.FP32, precision.OS_BN}}
    assert precision.current() is None
    with pytest.raises(KeyError):
        with precision.bf16_inference(None, Table()):
            raise KeyError("x")
    assert precision.current() is None


def test_the_rounding_helper_rounds_ties_to_even():
    """t.bfloat16().float() is what tests/test_gpu_bf16.py rounds its operands with: 8 significant bits, ties to even"""
    def rnd(v):
        return float(torch.tensor([v], dtype=torch.float32).bfloat16().float())
    assert rnd(1 + 2.0 ** -8) == 1.0                                   # tie between 1 and 1 + 2^-7: even is 1
    assert rnd(1 + 2.0 ** -7 + 2.0 ** -8) == 1 + 2.0 ** -6             # tie between 1 + 2^-7 and 1 + 2^-6: even is the latter
    assert rnd(1 + 2.0 ** -8 + 2.0 ** -20) == 1 + 2.0 ** -7            # above the tie: up
    assert rnd(1 + 2.0 ** -7 + 2.0 ** -8 - 2.0 ** -20) == 1 + 2.0 ** -7   # below the tie: down
    assert rnd(-(1 + 2.0 ** -8)) == -1.0
    z = torch.tensor([0.0, -0.0]).bfloat16()
    assert z.view(torch.int16).tolist() == [0, -32768]                 # the sign of a zero survives
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    assert float(((x.bfloat16().float() - x).abs() / x.abs()).max()) <= 2.0 ** -8      # unit roundoff of 8 significant bits
