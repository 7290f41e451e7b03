"""WholeBodyAE pre-training on the device: the hybrid data set, vatl_ae_backward behind loss.backward(), the fused large-batch step
and the trainer, against float64 / fp32 torch restatements on the CPU (oracle.nets.WholeBodyAERef) and tests/golden/wholebody.npz."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import nets
from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wholebody.npz")
DIGITS = {"Posetrack21": 2, "JRDB2022": 3}
JSON = {"Posetrack21": "PoseTrack21/activelearning/{m}/000000_integrated_{m}.json", "JRDB2022": "jrdb-pose/activelearning/{m}/integrated_{m}.json"}
# (x - centroid) / height cancels to rounding residue where a key-point sits on the centroid: person 10 of the JRDB list has x16 = 827.32 =
# centroid, the exact feature is 1.8e-16, the reference's own float64 result 4.2e-16 and the kernel's 0.  No relative bar applies to such an
# element, so the 1e-4 relative bar gets the absolute floor test_hybrid_feature_and_autoencoder_api already grants this function against the
# same reference (1e-13: ~500 ulp of a 1000-px coordinate over a 100-px box height); every other feature is O(0.01 .. 1), 1e9 times above it.
HYBRID_ATOL = 1e-13
GRAD_CASES = [(38, 5, 10000), (42, 2, 8000), (51, 5, 10000), (42, 4, 257), (38, 2, 1)]


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def annotations(g, dtype):
    return [{"id": int(i), "image_id": int(m), "bbox": b.tolist(), "keypoints": k.tolist()}
            for i, m, b, k in zip(g[f"{dtype}_id"], g[f"{dtype}_image_id"], g[f"{dtype}_bbox"], g[f"{dtype}_keypoints"])]


def ann_id(a, dtype):
    return int(str(int(a["id"]))[-DIGITS[dtype]:] + str(a["image_id"]))


def write_json(root, dtype, mode, anns):
    path = os.path.join(root, JSON[dtype].format(m=mode))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"annotations": anns}, f)


def pair(d, z, seed=0):
    """A default-initialised float32 reference network and a WholeBodyAE on the device holding the same weights."""
    from active_learning.Whole_body_AE import WholeBodyAE
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        ref = nets.WholeBodyAERef(z_dim=z, input_dim=d)
    ae = WholeBodyAE(z_dim=z, input_dim=d)
    ae.load_state_dict(ref.state_dict())
    return ref, ae.to(dev())


def uniform(n, d, seed):
    return np.random.RandomState(seed).uniform(0, 1, (n, d)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. hybrid data set
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", list(DIGITS))
def test_hybrid_dataset_matches_the_references_features(golden, tmp_path, dtype):
    from active_learning.Whole_body_AE import Wholebody
    root = str(tmp_path / "data")
    anns = annotations(golden, dtype)
    write_json(root, dtype, "train", anns)
    ds = Wholebody("train", dataset_type=dtype, data_root=root)
    order = sorted((k for k, a in enumerate(anns) if sum(a["keypoints"][2::3]) != 0), key=lambda k: ann_id(anns[k], dtype))
    want = golden[f"{dtype}_hybrid"][order]
    assert len(ds) == int(golden[f"{dtype}_ref_len"]) == len(order)
    assert [it["ann_id"] for it in ds.items] == [ann_id(anns[k], dtype) for k in order]
    got = np.stack([np.asarray(it["feature"]) for it in ds.items])
    assert got.shape == (len(order), 42) and got.dtype == np.float64
    record(f"wholebody_hybrid_{dtype}", max_rel=float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=HYBRID_ATOL)
    for i in range(len(ds)):
        item = ds[i]
        assert item.dtype == torch.float32 and item.device.type == "cpu"
        np.testing.assert_allclose(item.numpy(), want[i].astype(np.float32), rtol=1e-4, atol=HYBRID_ATOL)
    last = max(k for k in order)                                     # the reference's element 0 = the last kept person in file order
    np.testing.assert_allclose(ds[order.index(last)].numpy(), golden[f"{dtype}_ref_item0_hybrid"], rtol=1e-4, atol=HYBRID_ATOL)
    ds38 = Wholebody("train", dataset_type=dtype, data_root=root, feature_dim=38)         # served by the cache written above
    assert all(torch.equal(ds38[i], ds[i][:38]) for i in range(len(ds)))
    assert torch.equal(ds38.features(), ds.features()[:, :38]) and ds.features().shape == (len(order), 42)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. gradients through loss.backward()
# ---------------------------------------------------------------------------------------------------------------------------------

def f64_grads(ref, x, x_grad=False):
    r64 = nets.WholeBodyAERef(z_dim=ref.encoder[6].out_features, input_dim=ref.encoder[0].in_features)
    r64.load_state_dict(ref.state_dict())
    r64 = r64.double()
    x64 = torch.from_numpy(x).double().requires_grad_(x_grad)
    loss = torch.nn.MSELoss()(r64(x64), x64)
    loss.backward()
    return loss.item(), [p.grad.numpy() for p in r64.parameters()], (x64.grad.numpy() if x_grad else None)


def check_grads(name, d, z, n):
    ref, ae = pair(d, z, seed=d * 100 + z)
    x = uniform(n, d, seed=n)
    ae.train()
    xd = to_dev(x)
    loss = torch.nn.MSELoss()(ae(xd), xd)
    loss.backward()
    want_loss, want, _ = f64_grads(ref, x)
    print(f"{name}: loss {loss.item():.9g} vs {want_loss:.9g}")
    worst = 0.0
    for (k, p), g in zip(ae.named_parameters(), want):
        assert p.grad is not None and p.grad.shape == p.shape, k
        e = rel_err(p.grad.cpu().numpy(), g)
        print(f"{name}: {k} rel_err {e:.3e}")
        worst = max(worst, e)
    record(name, worst_grad_rel=worst, loss_rel=abs(loss.item() - want_loss) / want_loss)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=1e-5)
    for (k, p), g in zip(ae.named_parameters(), want):
        assert rel_err(p.grad.cpu().numpy(), g) < 2e-5, k
    return ref, ae, x, xd


@pytest.mark.parametrize("d,z,n", GRAD_CASES)
def test_gradients_match_float64_autograd(vh, d, z, n):
    ref, ae, x, xd = check_grads(f"ae_backward_d{d}_z{z}_n{n}", d, z, n)
    first = [p.grad.clone() for p in ae.parameters()]
    ae.zero_grad(set_to_none=True)
    torch.nn.MSELoss()(ae(xd), xd).backward()                        # a second identical call: identical bits
    assert all(torch.equal(a, p.grad) for a, p in zip(first, ae.parameters()))
    # the gradient w.r.t. the input, when it asks for one
    ae.zero_grad(set_to_none=True)
    xg = to_dev(x).requires_grad_()
    torch.nn.MSELoss()(ae(xg), xg).backward()
    _, _, want_dx = f64_grads(ref, x, x_grad=True)
    e = rel_err(xg.grad.cpu().numpy(), want_dx)
    print(f"dx rel_err {e:.3e}")
    assert xg.grad.shape == (n, d) and e < 2e-5
    assert all(torch.equal(a, p.grad) for a, p in zip(first, ae.parameters()))             # asking for dx does not change the others
    # forward values: the train-mode path, eval() and no_grad() all return vatl_ae_forward's bits
    want_y, _ = vh.ae_forward(xd, vh.pack_ae(ae.state_dict(), dev()), d, z)
    assert torch.equal(ae(xd).detach(), want_y)
    with torch.no_grad():
        assert torch.equal(ae(xd), want_y) and not ae(xd).requires_grad
    ae.eval()
    assert torch.equal(ae(xd), want_y) and ae(xd).grad_fn is None
    ae.train()
    for p in ae.parameters():
        p.requires_grad_(False)
    assert ae(xd).grad_fn is None                                    # nothing to differentiate: today's path


def test_gradients_of_a_batch_whose_blocks_walk_several_chunks(vh):
    """Above 65 536 rows a block takes more than one 64-item chunk and carries its sums across them (beyond the sizes the
    pre-training loop uses; same bound)."""
    check_grads("ae_backward_d38_z2_n70001", 38, 2, 70001)


def test_forward_refuses_wrong_width_and_cpu_tensors(vh):
    from active_learning.Whole_body_AE import WholeBodyAE
    ae = WholeBodyAE(z_dim=5).to(dev()).train()                      # the released default: 38 inputs
    with pytest.raises(vh.VatlError, match="§9 item 1"):
        ae(to_dev(uniform(76, 42, 1)))                               # 76 x 42 = 84 x 38: must not be reshaped into nonsense
    ae.eval()
    with pytest.raises(vh.VatlError, match="§9 item 1"):
        ae(to_dev(uniform(19, 42, 1)))
    for mode in (ae.train, ae.eval):
        mode()
        with pytest.raises(vh.VatlError):
            ae(torch.zeros(4, 38))
    ws = vh.ae_grad_workspace(16, 38, 5, dev())
    flat = vh.pack_ae(ae.state_dict(), dev()).clone()
    x = to_dev(uniform(16, 38, 2))
    for bad in (lambda: vh.lib().vatl_ae_backward(x.data_ptr(), x.data_ptr(), flat.data_ptr(), 65, 5, 16, flat.data_ptr(), None, ws.data_ptr(), None),
                lambda: vh.lib().vatl_ae_backward(x.data_ptr(), x.data_ptr(), flat.data_ptr(), 38, 5, 0, flat.data_ptr(), None, ws.data_ptr(), None),
                lambda: vh.lib().vatl_ae_backward(x.data_ptr(), x.data_ptr(), flat.data_ptr(), 38, 5, 16, flat.data_ptr(), None, None, None),
                lambda: vh.lib().vatl_ae_train_step_large(flat.data_ptr(), flat.data_ptr(), flat.data_ptr(), x.data_ptr(), 16, 38, 5, 1e-3, 0.9, 0.999,
                                                          1e-8, 0.01, 0, 1, None, ws.data_ptr(), None),
                lambda: vh.lib().vatl_ae_train_step_large(flat.data_ptr(), flat.data_ptr(), flat.data_ptr(), x.data_ptr(), 16, 38, 5, 1e-3, 0.9, 0.999,
                                                          1e-8, 0.01, 1, 2, None, ws.data_ptr(), None)):
        assert bad() == -1 and vh.lib().vatl_last_error()            # VATL_EINVAL, nothing launched
    assert vh.lib().vatl_ae_grad_workspace_floats(0, 38, 5) == 0 and vh.lib().vatl_ae_grad_workspace_floats(16, 38, 65) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. fused step
# ---------------------------------------------------------------------------------------------------------------------------------

D6, Z6, ROWS6, LR6 = 42, 5, 25000, 1e-3


def schedule6(seed=6):
    g = torch.Generator()
    g.manual_seed(seed)
    for _ in range(4):
        perm = torch.randperm(ROWS6, generator=g)
        for i in range(0, ROWS6, 10000):
            yield perm[i:i + 10000]


def fused_run(vh, ae, data, decoupled):
    flat = vh.pack_ae(ae.state_dict(), dev()).clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    losses = []
    for step, idx in enumerate(schedule6(), 1):
        losses.append(vh.ae_train_step_large(flat, m, v, data[idx.to(dev())].contiguous(), D6, Z6, step, LR6, decoupled=decoupled,
                                             weight_decay=0.01 if decoupled else 0.0))
    return flat, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_fused_step_matches_torch_optimizer(vh, decoupled):
    ref, ae = pair(D6, Z6, seed=61)
    x = uniform(ROWS6, D6, seed=62)
    xt, data = torch.from_numpy(x), to_dev(x)
    flat, losses = fused_run(vh, ae, data, decoupled)
    assert len(losses) == 12
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref.parameters(), lr=LR6)
    want = []
    for idx in schedule6():
        b = xt[idx]
        loss = torch.nn.MSELoss()(ref(b), b)
        opt.zero_grad(); loss.backward(); opt.step()
        want.append(loss.item())
    print("losses", losses.tolist(), "want", want)
    got_p = flat.cpu().numpy()
    want_p = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).numpy()
    diff = np.abs(got_p - want_p)
    print(f"median |dp| {np.median(diff):.3e}  max |dp| {diff.max():.3e}")
    record(f"ae_train_step_large_{'adamw' if decoupled else 'adam'}", loss_rel=float(np.max(np.abs(losses - want) / np.abs(want))),
           median_abs=float(np.median(diff)), max_abs=float(diff.max()))
    np.testing.assert_allclose(losses, want, rtol=1e-5)
    assert np.median(diff) < 1e-6
    assert diff.max() <= LR6 * 12
    again, losses2 = fused_run(vh, ae, data, decoupled)              # the same 12 steps: identical bits
    assert torch.equal(again, flat) and np.array_equal(losses, losses2)


def test_autograd_path_and_fused_path_agree(vh):
    ref, ae = pair(D6, Z6, seed=61)
    data = to_dev(uniform(ROWS6, D6, seed=62))
    _, fused = fused_run(vh, ae, data, True)
    ae.train()
    opt = torch.optim.AdamW(ae.parameters(), lr=LR6)
    got = []
    for step, idx in zip(range(3), schedule6()):
        b = data[idx.to(dev())]
        loss = torch.nn.MSELoss()(ae(b), b)
        opt.zero_grad(); loss.backward(); opt.step()
        got.append(loss.item())
    print("autograd", got, "fused", fused[:3].tolist())
    np.testing.assert_allclose(got, fused[:3], rtol=1e-5)


def test_fit_autoencoder_takes_large_batches(vh):
    from active_learning.Whole_body_AE.AutoEncoder import fit_autoencoder
    _, ae = pair(42, 4, seed=63)
    feats = to_dev(np.random.RandomState(3).uniform(0.2, 0.8, (500, 42)).astype(np.float32))
    with torch.no_grad():
        before = float(((ae(feats) - feats) ** 2).mean())
    g = torch.Generator(); g.manual_seed(0)
    mean_loss = fit_autoencoder(ae, feats, epochs=20, lr=1e-2, batch_size=200, generator=g)
    with torch.no_grad():
        after = float(((ae(feats) - feats) ** 2).mean())
    assert after < before and np.isfinite(mean_loss)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. trainer
# ---------------------------------------------------------------------------------------------------------------------------------

def script_loop(ref, train, valid, epochs, seed):
    """wholebodyAE_train.py:118-176 restated on the CPU in fp32: the losses it logs, the best epoch and the learning rates."""
    opt = torch.optim.AdamW(ref.parameters(), lr=0.001)
    crit = torch.nn.MSELoss()
    g = torch.Generator(); g.manual_seed(seed)
    log = {"Train_loss": [], "Valid_loss": []}
    best_loss = 0
    for epoch in range(epochs):
        if epoch == 12:
            opt.param_groups[0]["lr"] = 0.0002
        if epoch == 40:
            opt.param_groups[0]["lr"] = 0.00005
        perm = torch.randperm(train.shape[0], generator=g)
        tl, nb = 0.0, 0
        for i in range(0, train.shape[0], 10000):
            b = train[perm[i:i + 10000]]
            loss = crit(ref(b), b)
            tl += loss.item(); nb += 1
            opt.zero_grad(); loss.backward(); opt.step()
        log["Train_loss"].append(tl / nb)
        vl, nvb = 0.0, 0
        with torch.no_grad():
            for i in range(0, valid.shape[0], 8000):
                b = valid[i:i + 8000]
                vl += crit(ref(b), b).item(); nvb += 1
        log["Valid_loss"].append(vl / nvb)
        if vl < best_loss or epoch == 0:
            best_loss = vl
            log["best_epoch"], log["best_loss"] = epoch, best_loss / nvb
    return log


def test_trainer_end_to_end(vh, golden, tmp_path):
    from active_learning import driver_paths
    from active_learning.Whole_body_AE import WholeBodyAE
    from active_learning.Whole_body_AE.pretrain import pretrain_autoencoder
    from alphapose.utils.config import edict
    z = 5
    ref, ae = pair(42, z, seed=71)
    train, valid = torch.from_numpy(uniform(25000, 42, seed=72)), torch.from_numpy(uniform(12000, 42, seed=73))
    save_root = str(tmp_path / "run")
    res = pretrain_autoencoder(train, valid, z, epochs=4, save_root=save_root, seed=318, model=ae)
    want = script_loop(ref, train, valid, 4, seed=318)
    log = json.load(open(os.path.join(save_root, "log.json")))
    print("log", log, "want", want)
    assert set(log) == {"z_dim", "epoch", "pretrained", "kp_direct", "Train_loss", "Valid_loss", "best_epoch", "best_loss"}
    assert (log["z_dim"], log["epoch"], log["pretrained"], log["kp_direct"]) == (z, 4, False, False)
    np.testing.assert_allclose(log["Train_loss"], want["Train_loss"], rtol=1e-5)
    np.testing.assert_allclose(log["Valid_loss"], want["Valid_loss"], rtol=1e-5)
    best, best_loss = 0, log["Valid_loss"][0]                         # the script's rule on the logged values: epoch 0, then `valid < best`
    for e, vl in enumerate(log["Valid_loss"]):
        if vl < best_loss:
            best, best_loss = e, vl
    assert log["best_epoch"] == best == want["best_epoch"]
    np.testing.assert_allclose(log["best_loss"], best_loss, rtol=1e-12)
    assert res["lr"] == [1e-3] * 4 and res["log"] == log
    sd = torch.load(os.path.join(save_root, f"WholeBodyAE_zdim{z}.pth"))
    assert list(sd) == list(ref.state_dict()) and len(sd) == 16
    assert all(isinstance(v, torch.Tensor) and v.device.type == "cpu" and v.dtype == torch.float32 for v in sd.values())
    if best == 3:                                                    # the best epoch is the last: the file holds the final weights
        for k, v in res["model"].state_dict().items():
            assert torch.equal(v.cpu(), sd[k])
        got_p = torch.cat([v.reshape(-1) for v in sd.values()]).numpy()
        want_p = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).numpy()
        assert np.median(np.abs(got_p - want_p)) < 1e-6
    # the driver finds the file where ActiveLearning.initialize_AE looks for it, and WPU scores poses with it
    root = tmp_path / "pretrained"
    os.makedirs(root / "Hybrid")
    torch.save(sd, root / "Hybrid" / f"WholeBodyAE_zdim{z}.pth")
    cfg = edict({"AE": {"PRETRAINED_ROOT": str(root), "Z_DIM": z}})
    path = driver_paths.resolve_ae_checkpoint(cfg)
    assert path == os.path.join(str(root), "Hybrid", f"WholeBodyAE_zdim{z}.pth")
    loaded, input_dim, z_dim = driver_paths.load_ae_checkpoint(path, cfg)
    assert (input_dim, z_dim) == (42, z) == (loaded["encoder.0.weight"].shape[1], z)
    scorer = WholeBodyAE(z_dim=z_dim, input_dim=input_dim)
    scorer.load_state_dict(loaded, strict=True)
    keep = ~np.isnan(golden["Posetrack21_hybrid"][:, 0])
    kp = golden["Posetrack21_keypoints"][keep].reshape(-1, 17, 3)
    bb = golden["Posetrack21_bbox"][keep]
    xyxy = np.stack([bb[:, 0], bb[:, 1], bb[:, 0] + bb[:, 2], bb[:, 1] + bb[:, 3]], 1)
    wpu, status = vh.hybrid_ae_wpu(to_dev(kp), to_dev(xyxy), vh.pack_ae(scorer.state_dict(), dev()), input_dim, z_dim)
    assert not status.cpu().numpy().any() and np.isfinite(wpu.cpu().numpy()).all() and wpu.shape == (int(keep.sum()),)


def test_trainer_learning_rate_changes_at_epoch_12(vh):
    from active_learning.Whole_body_AE.pretrain import pretrain_autoencoder
    res = pretrain_autoencoder(uniform(300, 42, 1), uniform(100, 42, 2), 2, epochs=13)
    assert res["lr"] == [1e-3] * 12 + [2e-4] and len(res["log"]["Train_loss"]) == 13 and res["checkpoint"] is None
    assert res["model"].input_dim == 42 and res["model"].z_dim == 2
    res38 = pretrain_autoencoder(uniform(300, 42, 1), uniform(100, 42, 2), 2, input_dim=38, epochs=1)
    assert res38["model"].input_dim == 38


def test_main_trains_on_raw_keypoints(vh, golden, tmp_path, monkeypatch):
    from active_learning.Whole_body_AE import pretrain
    anns = annotations(golden, "Posetrack21")
    write_json(str(tmp_path / "data"), "Posetrack21", "train", anns)
    write_json(str(tmp_path / "data"), "Posetrack21", "train_val", anns[:20])
    monkeypatch.chdir(tmp_path)
    res = pretrain.main(["--dataset_type", "Posetrack21", "--kp_direct", "--z", "5", "--epoch", "2"])
    assert res["model"].input_dim == 51 and len(res["log"]["Train_loss"]) == 2 and res["log"]["kp_direct"] is True
    assert res["checkpoint"].startswith("exp/Whole_body_AE/Posetrack21/direct/zdim_5/") and os.path.isfile(res["checkpoint"])
    sd = torch.load(res["checkpoint"])
    assert sd["encoder.0.weight"].shape == (24, 51) and sd["decoder.6.bias"].shape == (51,)
    assert os.path.isfile(os.path.join(os.path.dirname(res["checkpoint"]), "log.json"))
    assert np.isfinite(res["log"]["Train_loss"]).all() and np.isfinite(res["log"]["Valid_loss"]).all()
