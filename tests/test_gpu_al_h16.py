"""`cfg.VAL.PRECISION`: the evaluation pass of an active-learning round on the opt-in 16-bit route (fp16 / bf16), the default untouched.
The config and options are those of tests/test_gpu_al.py (seeded SyntheticVideo, SimplePose-R50 from scratch, uncertainty THC+WPU)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import scorers
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu


def _cfg(precision=None):
    from alphapose.utils.config import edict
    val = {"BATCH_SIZE": 10, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.25, 0.5, 1.0]}
    if precision is not None:
        val["PRECISION"] = precision
    return edict({
        "DATASET": {"TRAIN": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 24, "TRACKS": 2}, "EVAL": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 24, "TRACKS": 2}},
        "DATA_PRESET": {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]},
        "MODEL": {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50},
        "LOSS": {"TYPE": "MSELoss"},
        "AE": {"Z_DIM": 4, "INPUT_DIM": 42, "PRETRAINED": "", "EPOCH": 2, "LR": 1e-3},
        "RETRAIN": {"BATCH_SIZE": 8, "BASE": 1, "OPTIMIZER": "AdamW", "LR": 2.5e-4, "ALPHA": 2, "WEIGHT_DECAY": 0.7, "LR_GAMMA": 0.99},
        "VAL": val,
    })


def _opt(work_dir=None):
    unc = "THC+WPU"
    return types.SimpleNamespace(work_dir=work_dir, uncertainty=unc, representativeness="None", filter="None", strategy=unc, video_id="syn", get_prenext=True,
                                 from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const")


def _first_round(precision, work_dir=None):
    from active_learning import ActiveLearning
    torch.manual_seed(0)
    np.random.seed(0)
    al = ActiveLearning(_cfg(precision), _opt(work_dir))
    al.eval_and_query()
    return al


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_evaluation_pass_on_the_16_bit_route(precision, tmp_path):
    from alphapose.models import hip_engine_h16
    al = _first_round(precision, str(tmp_path))
    assert al.precision == precision and al.precision_dtype is {"fp16": torch.float16, "bf16": torch.bfloat16}[precision]
    assert np.isfinite(al.keypoints).all() and np.isfinite(al.oks).all()
    assert len(al.labeled_id) == 6 and len(al.unlabeled_id) == 18
    # the stream scorer agrees with the per-item oracle on the heat-maps the 16-bit route itself produces
    ds = al.eval_dataset
    al.model.eval()
    hm = hip_engine_h16.forward_h16(al.model, torch.stack([ds[i][1][0] for i in range(4)]).to(dev()), dtype=al.precision_dtype).cpu().numpy()
    for i in range(4):
        d = scorers.decode_heatmaps(hm[i], ds.bbox[i])
        np.testing.assert_allclose(al.keypoints[i].reshape(17, 3)[:, :2], d["coords"], rtol=1e-4, atol=1e-4)
    u = al.uncertainty_dict["Round0"]
    assert all(np.isfinite(np.asarray(u[i], np.float64)).all() for i in range(24))
    assert al.performance[0]["precision"] == precision and al.performance[0]["AP"] is None and 0.0 <= al.performance[0]["mOKS"] <= 1.0
    al.flush_records()
    recs = json.load(open(os.path.join(str(tmp_path), "predicted_kpt.json")))
    assert len(recs) == 24 and np.isfinite(np.asarray([r["keypoints"] for r in recs])).all()
    np.testing.assert_allclose(recs[3]["keypoints"], al.keypoints[3], rtol=1e-6)
    assert al.outcome() is None and np.isfinite(al.last_train_loss)            # the fine-tune stays fp32
    al.close()


def test_embeddings_come_from_the_same_16_bit_trunk_pass():
    """Representativeness "Influence" needs get_embedding: with PRECISION = fp16 it comes from `forward_with_embedding_h16`, and the influence
    scores are the sklearn restatement's on `embedding_h16`'s vectors (rtol as tests/test_gpu_al.py holds the fp32 path to its own embeddings)."""
    from active_learning import ActiveLearning
    from alphapose.models import hip_engine_h16
    from oracle import query as OQ
    opt = types.SimpleNamespace(uncertainty="THC_L1", representativeness="Influence", filter="None", strategy="THC_L1", video_id="syn", get_prenext=True,
                                from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const", fixed_lambda=False)
    torch.manual_seed(0)
    np.random.seed(0)
    al = ActiveLearning(_cfg("fp16"), opt)
    al.eval_and_query()
    ds = al.eval_dataset
    al.model.eval()
    emb = hip_engine_h16.embedding_h16(al.model, torch.stack([ds[i][1][0] for i in range(24)]).to(dev()), dtype=torch.float16).cpu().numpy()
    assert emb.dtype == np.float32 and np.isfinite(emb).all()
    inf = al.influence_dict["Round0"]
    np.testing.assert_allclose([inf[i] for i in range(24)], OQ.influence_scores(emb), rtol=1e-6, atol=1e-9)
    assert len(al.query_list_list["Round0"]) == 6 and al.performance[0]["precision"] == "fp16"
    al.close()


def test_fp32_and_an_absent_key_are_the_same_run():
    a, b = _first_round(None), _first_round("fp32")
    assert a.precision == b.precision == "fp32" and a.precision_dtype is None and b.precision_dtype is None
    assert np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.oks, b.oks)
    ua, ub = a.uncertainty_dict["Round0"], b.uncertainty_dict["Round0"]
    assert sorted(ua) == sorted(ub) and all(np.array_equal(np.asarray(ua[k]), np.asarray(ub[k])) for k in ua)
    assert a.query_list_list["Round0"] == b.query_list_list["Round0"]
    assert "precision" not in a.performance[0] and a.performance[0] == b.performance[0]
    a.close(); b.close()


def test_an_unknown_precision_is_refused_by_the_constructor():
    from active_learning import ActiveLearning
    with pytest.raises(ValueError, match="PRECISION"):
        ActiveLearning(_cfg("fp8"), _opt())
