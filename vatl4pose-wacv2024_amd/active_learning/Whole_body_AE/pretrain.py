"""Pre-training of the whole-body auto-encoder, resident on the device (what scripts/wholebodyAE_train.py:110-184 does through
``DataLoader``, autograd and ``torch.optim.AdamW``).

    python -m active_learning.Whole_body_AE.pretrain --dataset_type Posetrack21 [--z 5] [--epoch 80] [--pretrained] [--kp_direct] [--input_dim 38]

writes ``exp/Whole_body_AE/<dataset_type>/<hybrid|direct>/zdim_<Z>/<time>/WholeBodyAE_zdim<Z>.pth`` (the file
``ActiveLearning.initialize_AE`` looks for under ``<AE.PRETRAINED_ROOT>/Hybrid/``) and ``log.json`` with the script's keys.

The loop keeps the script's behaviour: AdamW (weight decay 0.01) at 1e-3, 2e-4 from epoch 12, 5e-5 from epoch 40; batches of 10 000
(train, shuffled) and 8 000 (validation), the last one ragged; early stopping with patience 30 on the SUM of the validation batch
losses; "best" when ``valid_loss < best_loss or epoch == 0``.  What differs is where it runs: the features are uploaded once, each
epoch draws one ``torch.randperm`` from a seeded CPU generator, every train batch is one ``vatl_ae_train_step_large`` call,
validation reads ``vatl_ae_forward``'s per-item MSE, and the batch losses stay on the device until ONE read-back per epoch.
``input_dim`` defaults to the width of the features (42 for hybrid features: SURVEY.md §9 item 1); a smaller value trains on the
leading columns, as ``retrain_AE`` does.  Plots are not written.
"""
from __future__ import annotations

import argparse
import datetime
import json
import os

import torch

import vatl_hip as vh

from .AutoEncoder import WholeBodyAE

TRAIN_BATCH, VALID_BATCH = 10000, 8000
WEIGHT_DECAY = 0.01                                   # torch.optim.AdamW's default: the script passes none
PATIENCE = 30


def learning_rate(epoch: int) -> float:
    return 5e-5 if epoch >= 40 else (2e-4 if epoch >= 12 else 1e-3)


class EarlyStopping:
    """The script's rule: stop once the validation loss has failed to improve ``patience`` epochs in a row."""

    def __init__(self, patience: int = 5):
        self.patience, self.counter, self.best_loss, self.early_stop = patience, 0, None, False

    def __call__(self, valid_loss: float) -> bool:
        if self.best_loss is None:
            self.best_loss = valid_loss
        elif self.best_loss - valid_loss > 0:
            self.best_loss, self.counter = valid_loss, 0
        else:
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True
        return self.early_stop


def _resident(feats, input_dim, device) -> torch.Tensor:
    t = torch.as_tensor(feats)
    t = t.reshape(t.shape[0], -1)
    if input_dim is not None:
        if t.shape[1] < input_dim:
            raise vh.VatlError(f"features are {t.shape[1]} wide, input_dim = {input_dim} asks for more")
        t = t[:, :input_dim]
    return vh.upload(t.contiguous(), device, torch.float32).contiguous()


def cpu_state_dict(model: WholeBodyAE) -> dict:
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def pretrain_autoencoder(train_feats, valid_feats, z_dim, input_dim=None, epochs=80, save_root=None, seed=318, generator=None, model=None,
                         log_meta=None, device=None):
    """Train a ``WholeBodyAE`` on ``train_feats`` (N, W), validate on ``valid_feats`` (M, W).  ``generator`` is the CPU generator of
    the epoch permutations (default: a new one seeded with ``seed``); ``model`` a module to continue from (default: a new one whose
    initial weights are drawn under ``torch.manual_seed(seed)`` without disturbing the global generator).  With ``save_root`` the best
    checkpoint and ``log.json`` are written there.  Returns {"model", "log", "lr" (one value per epoch run), "checkpoint"}."""
    if not torch.cuda.is_available():
        raise vh.VatlError("the auto-encoder trains on MI355X only (no CPU fallback)")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if input_dim is None:
        input_dim = int(model.input_dim) if model is not None else int(torch.as_tensor(train_feats).reshape(len(train_feats), -1).shape[1])
    train, valid = _resident(train_feats, input_dim, device), _resident(valid_feats, input_dim, device)
    n, nv = train.shape[0], valid.shape[0]
    if n == 0 or nv == 0:
        raise vh.VatlError(f"pre-training needs train and validation rows (got {n} and {nv})")
    if model is None:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            model = WholeBodyAE(z_dim=z_dim, input_dim=input_dim)
    if (model.input_dim, model.z_dim) != (input_dim, z_dim):
        raise vh.VatlError(f"model is {model.input_dim} -> {model.z_dim}, asked for {input_dim} -> {z_dim}")
    model = model.to(device)
    if generator is None:
        generator = torch.Generator()
        generator.manual_seed(seed)

    flat = vh.pack_ae(model.state_dict(), device).clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    nb, nvb = -(-n // TRAIN_BATCH), -(-nv // VALID_BATCH)
    losses = torch.zeros(nb + nvb, device=device, dtype=torch.float32)          # this epoch's batch losses: train, then validation
    spaces = {}                                                                # batch rows -> block-partial workspace

    def workspace(rows):
        if rows not in spaces:
            spaces[rows] = vh.ae_grad_workspace(rows, input_dim, z_dim, device)
        return spaces[rows]

    meta = log_meta or {}
    log = {"z_dim": z_dim, "epoch": epochs, "pretrained": bool(meta.get("pretrained", False)), "kp_direct": bool(meta.get("kp_direct", False)),
           "Train_loss": [], "Valid_loss": []}
    stopper, best_loss, step, lrs, checkpoint = EarlyStopping(PATIENCE), 0, 0, [], None
    if save_root is not None:
        os.makedirs(save_root, exist_ok=True)
    for epoch in range(epochs):
        lr = learning_rate(epoch)
        lrs.append(lr)
        shuffled = train[torch.randperm(n, generator=generator, device="cpu").to(device)]
        for k, i in enumerate(range(0, n, TRAIN_BATCH)):
            step += 1
            batch = shuffled[i:i + TRAIN_BATCH]
            vh.ae_train_step_large(flat, m, v, batch, input_dim, z_dim, step, lr, weight_decay=WEIGHT_DECAY, decoupled=True,
                                   workspace=workspace(batch.shape[0]), loss=losses[k:k + 1])
        for k, i in enumerate(range(0, nv, VALID_BATCH)):
            _, mse = vh.ae_forward(valid[i:i + VALID_BATCH], flat, input_dim, z_dim, want_recon=False)
            losses[nb + k] = mse.double().mean()                               # equal widths: the mean of the row means is MSELoss
        sums = torch.stack([losses[:nb].double().sum(), losses[nb:].double().sum()]).cpu()      # the epoch's one read-back
        train_loss, valid_loss = float(sums[0]), float(sums[1])
        log["Train_loss"].append(train_loss / nb)
        log["Valid_loss"].append(valid_loss / nvb)
        print(f"Epoch: {epoch + 1}, train_loss: {train_loss / nb: 0.4f}, val_loss: {valid_loss / nvb: 0.4f}")
        if stopper(valid_loss):
            print("Early Stopping!")
            break
        if valid_loss < best_loss or epoch == 0:
            best_loss = valid_loss
            log["best_epoch"], log["best_loss"] = epoch, best_loss / nvb
            if save_root is not None:
                vh.unpack_ae(flat, model)
                checkpoint = os.path.join(save_root, f"WholeBodyAE_zdim{z_dim}.pth")
                torch.save(cpu_state_dict(model), checkpoint)
    vh.unpack_ae(flat, model)
    for p in model.parameters():                                               # in-place update through the C ABI: bump the version counters
        torch.autograd.graph.increment_version(p)
    if save_root is not None:
        with open(os.path.join(save_root, "log.json"), "w") as f:
            json.dump(log, f)
    return {"model": model, "log": log, "lr": lrs, "checkpoint": checkpoint}


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="WholeBodyAE pre-training on MI355X")
    parser.add_argument("--z", type=int, default=5, help="dimension of latent space")
    parser.add_argument("--epoch", type=int, default=80, help="number of epochs")
    parser.add_argument("--pretrained", action="store_true", help="continue from pretrained_models/Whole_body_AE/<dataset_type>/zdim_<Z>.pth")
    parser.add_argument("--kp_direct", action="store_true", help="train on the 51 raw key-point values instead of hybrid features")
    parser.add_argument("--dataset_type", type=str, required=True, choices=["Posetrack21", "JRDB2022"], help="which dataset to use")
    parser.add_argument("--input_dim", type=int, default=None, help="train on the leading INPUT_DIM feature values (default: all of them)")
    return parser.parse_args(argv)


def main(argv=None):
    from .Whole_body_hybrid import Wholebody
    opt = parse_args(argv)
    kind = "direct" if opt.kp_direct else "hybrid"
    now = datetime.datetime.now().strftime("%Y-%m-%d_%H:%M:%S")
    save_root = f"exp/Whole_body_AE/{opt.dataset_type}/{kind}/zdim_{opt.z}/{now}"
    train_set = Wholebody(mode="train", kp_direct=opt.kp_direct, dataset_type=opt.dataset_type, feature_dim=opt.input_dim)
    valid_mode = "train_val" if opt.dataset_type == "Posetrack21" else "val"
    valid_set = Wholebody(mode=valid_mode, kp_direct=opt.kp_direct, dataset_type=opt.dataset_type, feature_dim=opt.input_dim)
    print(f"train dataset: {len(train_set)}, valid dataset: {len(valid_set)}")
    train, valid = train_set.features(), valid_set.features()
    model = None
    if opt.pretrained:
        model = WholeBodyAE(z_dim=opt.z, input_dim=train.shape[1])
        model.load_state_dict(torch.load(f"pretrained_models/Whole_body_AE/{opt.dataset_type}/zdim_{opt.z}.pth", map_location="cpu"))
    res = pretrain_autoencoder(train, valid, opt.z, input_dim=train.shape[1], epochs=opt.epoch, save_root=save_root, model=model,
                               log_meta={"pretrained": opt.pretrained, "kp_direct": opt.kp_direct})
    print(f"log and checkpoint saved under {save_root}")
    return res


if __name__ == "__main__":
    main()
