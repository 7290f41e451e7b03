"""The opt-in 16-bit forward (alphapose/models/hip_engine_h16.py) refuses what it does not serve BEFORE the library is asked to compute
anything — no GPU is needed to see that — and leaves nothing behind that `hip_engine.invalidate` would have to drop."""
import pytest
import torch

PRESET = {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]}


def _build(cfg):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    return builder.build_sppe(edict(dict({"PRETRAINED": "", "TRY_LOAD": ""}, **cfg)), preset_cfg=edict(PRESET))


@pytest.fixture()
def no_library(monkeypatch):
    """Any call into libvatl_hip.so fails the test: the refusals must come first."""
    import vatl_hip

    def boom():
        raise AssertionError("the library was asked to compute")
    monkeypatch.setattr(vatl_hip, "lib", boom)
    return vatl_hip


@pytest.fixture(scope="module")
def fastpose():
    return _build({"TYPE": "FastPose", "NUM_LAYERS": 50}).eval()


def test_cpu_tensor_is_refused(no_library, fastpose):
    from alphapose.models import hip_engine_h16 as h16
    x = torch.zeros(1, 3, 256, 192)
    for dt in h16.DTYPES:
        for fn in (h16.forward_h16, h16.embedding_h16):
            with pytest.raises(no_library.VatlError, match="no CPU fallback"):
                fn(fastpose, x, dtype=dt)
        with pytest.raises(no_library.VatlError, match="no CPU fallback"):
            h16.features_h16(fastpose.preact.layer1[0], torch.zeros(1, 64, 8, 6), dtype=dt)
        with pytest.raises(no_library.VatlError, match="no CPU fallback"):
            h16.features_h16(fastpose.duc1, torch.zeros(1, 512, 4, 3), dtype=dt)
        with pytest.raises(no_library.VatlError, match="no CPU fallback"):
            h16.forward_with_embedding_h16(fastpose, x, torch.zeros(1, 17, 64, 48), torch.zeros(1, 2048), dtype=dt)


def test_training_mode_is_refused(no_library):
    from alphapose.models import hip_engine_h16 as h16
    m = _build({"TYPE": "SimplePose", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}).train()
    x = torch.zeros(1, 3, 256, 192)
    for fn in (h16.forward_h16, h16.embedding_h16):
        with pytest.raises(no_library.VatlError, match=r"model\.eval\(\)"):
            fn(m, x)
    with pytest.raises(no_library.VatlError, match=r"model\.eval\(\)"):
        h16.features_h16(m.preact, x)


@pytest.mark.parametrize("modulated", [False, True])
def test_deformable_model_is_refused_by_name(no_library, modulated):
    from alphapose.models import hip_engine_h16 as h16
    m = _build({"TYPE": "FastPose", "NUM_LAYERS": 50, "DCN": {"MODULATED": modulated, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False},
                "STAGE_WITH_DCN": [False, True, True, True]}).eval()
    x = torch.zeros(1, 3, 256, 192)
    for fn in (h16.forward_h16, h16.embedding_h16):
        with pytest.raises(NotImplementedError, match=r"preact\.layer2\.0"):
            fn(m, x)
    with pytest.raises(NotImplementedError, match="DCN"):
        h16.features_h16(m.preact.layer3[1], torch.zeros(1, 1024, 4, 3))


def test_other_inputs_are_refused(no_library, fastpose):
    from alphapose.models import hip_engine_h16 as h16
    x = torch.zeros(1, 3, 256, 192)
    for fn in (h16.forward_h16, h16.embedding_h16):
        with pytest.raises(no_library.VatlError, match="float16"):
            fn(fastpose, x, dtype=torch.float32)
    with pytest.raises(no_library.VatlError, match="float16"):
        h16.features_h16(fastpose.duc1, torch.zeros(1, 512, 4, 3), dtype=torch.float32)
    with pytest.raises(no_library.VatlError, match=r"\(N,C,H,W\)"):
        h16.forward_h16(fastpose, torch.zeros(3, 256, 192))
    with pytest.raises(no_library.VatlError, match="empty batch"):
        h16.forward_h16(fastpose, torch.zeros(0, 3, 256, 192))


def test_invalidate_without_a_16_bit_plan_is_harmless(no_library, fastpose):
    """Nothing is cached across 16-bit calls: there is nothing for invalidate to drop, before or after a refused call."""
    from alphapose.models import hip_engine, hip_engine_h16 as h16
    before = {id(mod): set(mod.__dict__) for mod in fastpose.modules()}
    hip_engine.invalidate(fastpose)
    with pytest.raises(no_library.VatlError):
        h16.forward_h16(fastpose, torch.zeros(1, 3, 256, 192))
    hip_engine.invalidate(fastpose)
    assert {id(mod): set(mod.__dict__) for mod in fastpose.modules()} == before
