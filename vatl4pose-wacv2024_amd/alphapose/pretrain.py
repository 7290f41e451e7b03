"""Pre-training of the pose networks, resident on the device: what the reference's scripts/posetrack_train.py (and its twin
jrdbpose_train.py) does through ``alphapose.opt``, ``DataParallel``, autograd and ``torch.optim``.

    python -m alphapose.pretrain --cfg <yaml> --exp-id <id> [--snapshot 2] [--seed 0] [--workers 8] [--max-epochs N] [--validate-only CKPT]
                                 [--precision {fp32,bf16}] [--flip-test]

writes ``./exp/<exp-id>-<FILE_NAME>/`` with ``training.log``, ``model_<epoch>.pth``, ``model_best.pth``, ``final.pth`` and
``predicted_kpt.json`` — the files ``MODEL.PRETRAINED`` of the active-learning yamls names.

Kept from the reference (line numbers of posetrack_train.py unless another file is named):
* config: ``cfg = update_config(yaml)``, ``cfg.FILE_NAME`` = the yaml's base name, ``TRAIN.DPG_STEP`` shifted by ``DPG_MILESTONE``
  (opt.py:53-57), work dir ``./exp/<exp-id>-<FILE_NAME>/`` (opt.py:59), ``training.log`` with ``epochInfo``'s line (opt.py:78-84);
* model (``preset_model`` :215-234): ``PRETRAINED`` is a strict load, ``TRY_LOAD`` a name-and-shape filtered one, otherwise
  ``_initialize()``;
* optimiser and schedule (:155-161): ``'adam'`` / ``'rmsprop'`` at ``TRAIN.LR``, ``MultiStepLR(TRAIN.LR_STEP, TRAIN.LR_FACTOR)``;
* data (:165-167): ``build_dataset(cfg.DATASET.TRAIN, preset_cfg=cfg.DATA_PRESET, train=True)``, shuffled batches of
  ``TRAIN.BATCH_SIZE``, the ragged last one kept;
* training step (``train()`` :41-65): input ``inps[:, 0]``, loss ``0.5 * MSE(out*mask, label*mask)``, ``calc_accuracy`` of the masked
  tensors, batch-size weighted epoch averages (``DataLogger``), then the optimiser step;
* epoch loop (:173-212): ``BEGIN_EPOCH..END_EPOCH``, ``lr_scheduler.step()`` after each epoch; when ``(i+1) % snapshot == 0``
  ``model_<i>.pth``, validation, ``model_best.pth`` when the metric exceeds the best so far (0 at the start); at
  ``i == DPG_MILESTONE`` ``final.pth``, every group's lr back to ``TRAIN.LR`` and a new ``MultiStepLR(DPG_STEP, 0.1)``;
* validation (``validate_gt`` :89-133): ``DATASET.VAL`` with ``train=False``, batches of ``VAL.BATCH_SIZE``, ``m.eval()``, records
  ``bbox, image_id, ann_id, score = mean + 1.25*max, category_id, keypoints`` in ``<work_dir>/predicted_kpt.json``.

Deliberately different:
* No network call of any kind and no ``requests`` / ``tensorboardX`` / ``cachetools``: the reference POSTs to a LINE-Notify endpoint
  after every epoch (:182, :236-247); those messages are log lines here.
* One device, no ``DataParallel``.  Gradients land in the model's flat gradient arena only because its addresses persist (the
  optimiser's device table is built once); nothing is reduced across ranks.
* An unknown ``TRAIN.OPTIMIZER`` raises a ``ValueError`` naming it (the reference leaves ``optimizer`` unbound).
* The loss and accuracy read-backs are deferred as in ``ActiveLearning.retrain_model``: flushed at the end of each epoch and at
  least every ``FLUSH_EVERY`` steps.  No input gradient is computed.
* Worker counts never come from the number of CPUs the host shows: ``--workers`` (default 8, at most 16) sizes a thread pool
  that decodes the NEXT batch's frames while the device runs this one (Pillow releases the GIL); batches are made on the calling
  thread.
* DPG: the reference's DPG data set is broken in the reference itself and ours refuses ``dpg=True`` (coco_video.py), so after the
  milestone actions above training ENDS with a log line; ``final_DPG.pth`` is not written.  ``--max-epochs`` only shortens a run.
* Validation metric: ``evaluate_mAP`` (its ``AP``) when the COCO API is importable, otherwise 100 x the mean ``vatl_oks`` over
  the validation items; log and result name which (``val_metric``: "mAP" | "mOKS").  No AP arithmetic lives here.
  The decode is the batch kernel behind ``heatmap_to_coord_simple``.
* Checkpoints are CPU tensors under the reference's state-dict keys.
* ``TRAIN.PRECISION`` (absent = ``fp32``; ``--precision`` overrides it) chooses the training step's trainer: ``fp32`` is
  ``hip_train.trainer_for``, the bits of every shipped yaml; ``bf16`` is the opt-in step of ``hip_train_h16`` (SimplePose only: bf16
  storage and products, fp32 accumulation, gradients, master weights and optimiser state; every bf16 filter re-packed in one launch per
  step).  Only the trainer changes: the loss, the optimiser, the checkpoints (fp32 master weights) and the validation pass (the fp32
  engine; ``VAL.PRECISION`` is not read here) are the same.  Anything else — ``fp16`` would need loss scaling — is a ``ValueError``
  and ``bf16`` with another ``MODEL.TYPE`` a ``NotImplementedError``, both raised before a data set is built or the device is touched.
* ``VAL.FLIP_TEST`` (absent = ``false``; ``--flip-test`` switches it on) makes the validation pass run the mirrored crops as well and
  average the two heat-maps before the decode, as the reference's ``validate_gt`` does under its ``--flip-test``
  (``active_learning.ActiveLearning.flip_test``: the same key, function and refusals as the active-learning rounds).  The training step is
  untouched.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import vatl_hip as vh
from active_learning import optim
from alphapose.models import builder
from alphapose.utils.config import update_config
from alphapose.utils.metrics import DataLogger, calc_accuracy_begin, evaluate_mAP, have_coco_tools

PRECISIONS = ("fp32", "bf16")
FLUSH_EVERY = 50                                      # steps between read-backs of the pending losses / accuracies, at most
MAX_WORKERS = 16


# ---------------------------------------------------------------------------------------------------------------------
# configuration, files, log
# ---------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Pose-network pre-training on MI355X")
    parser.add_argument("--cfg", required=True, type=str, help="pre-training yaml")
    parser.add_argument("--exp-id", default="default", type=str, help="name of the run: the work dir is ./exp/<exp-id>-<yaml base name>/")
    parser.add_argument("--snapshot", default=2, type=int, help="checkpoint and validate every SNAPSHOT epochs (0 = never)")
    parser.add_argument("--seed", default=0, type=int, help="seed of the initial weights, the shuffling and the augmentation")
    parser.add_argument("--workers", default=8, type=int, help=f"threads decoding the next batch's frames ahead (0 = none, at most {MAX_WORKERS})")
    parser.add_argument("--max-epochs", default=None, type=int, help="stop after this many epochs of this run")
    parser.add_argument("--validate-only", default=None, type=str, metavar="CKPT", help="load CKPT (strict), validate, write predicted_kpt.json")
    parser.add_argument("--precision", default=None, choices=PRECISIONS, help="trainer of the training step; overrides the yaml's TRAIN.PRECISION (absent: fp32)")
    parser.add_argument("--flip-test", default=False, action="store_true", help="validate with the mirrored pass merged in; switches the yaml's VAL.FLIP_TEST on (absent: off)")
    return parser.parse_args(argv)


def load_config(path):
    """opt.py:53-57."""
    cfg = update_config(path)
    cfg["FILE_NAME"] = os.path.basename(path).split(".")[0]
    cfg.TRAIN.DPG_STEP = [i - cfg.TRAIN.DPG_MILESTONE for i in cfg.TRAIN.DPG_STEP]
    return cfg


def train_precision(cfg, override=None) -> str:
    """``override`` (the ``--precision`` flag) or ``cfg.TRAIN.PRECISION`` -> "fp32" (the default, and what an absent key means:
    ``hip_train.trainer_for``) or "bf16" (the opt-in step of ``hip_train_h16``, SimplePose only).  "fp16" would need loss scaling for the
    heat-map MSE gradients and is, like anything else, a ValueError; "bf16" with another network a NotImplementedError."""
    name = override if override is not None else (cfg.TRAIN.get("PRECISION", "fp32") if "TRAIN" in cfg else "fp32")
    if not isinstance(name, str) or name not in PRECISIONS:
        raise ValueError(f"TRAIN.PRECISION must be one of {sorted(PRECISIONS)}, got {name!r}")
    if name == "bf16":
        model = cfg.MODEL.get("TYPE")
        if model != "SimplePose":
            raise NotImplementedError(f"TRAIN.PRECISION bf16 serves SimplePose only, not MODEL.TYPE {model!r} (FastPose, DCN and HRNet train in fp32)")
    return name


def work_dir_for(exp_id, cfg) -> str:
    return "./exp/{}-{}/".format(exp_id, cfg.FILE_NAME)


def epoch_info(set_name, idx, loss, acc) -> str:
    """The line of ``logger.epochInfo`` (opt.py:78-84)."""
    return "{set}-{idx:d} epoch | loss:{loss:.8f} | acc:{acc:.4f}".format(set=set_name, idx=idx, loss=loss, acc=acc)


def make_logger(work_dir):
    """``training.log`` in the work dir plus the console, on a logger of this run's own (the reference configures the root logger)."""
    os.makedirs(work_dir, exist_ok=True)
    logger = logging.getLogger("alphapose.pretrain." + os.path.abspath(work_dir))
    logger.setLevel(logging.INFO)
    logger.propagate = False
    for h in list(logger.handlers):
        logger.removeHandler(h)
        h.close()
    logger.addHandler(logging.FileHandler(os.path.join(work_dir, "training.log")))
    logger.addHandler(logging.StreamHandler())
    return logger


def close_logger(logger):
    for h in list(logger.handlers):
        logger.removeHandler(h)
        h.close()


def cpu_state_dict(model) -> dict:
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------------
# model, optimiser
# ---------------------------------------------------------------------------------------------------------------------

def preset_model(cfg, log=print, build=None):
    """posetrack_train.py:215-234."""
    node = cfg.MODEL
    model = (build or builder.build_sppe)(node, preset_cfg=cfg.DATA_PRESET)
    if node.PRETRAINED:                                       # every key, every shape
        log(f"strict load of {node.PRETRAINED}")
        model.load_state_dict(torch.load(node.PRETRAINED, map_location="cpu"), strict=True)
    elif node.TRY_LOAD:                                       # what fits by name and shape; the rest keeps the module's own values
        own = model.state_dict()
        fits = {name: t for name, t in torch.load(node.TRY_LOAD, map_location="cpu").items()
                if name in own and tuple(t.shape) == tuple(own[name].shape)}
        log(f"filtered load of {node.TRY_LOAD}: {len(fits)} of {len(own)} tensors taken")
        own.update(fits)
        model.load_state_dict(own)
    else:
        log("new model: _initialize()")
        model._initialize()
    return model


def build_optimizer(cfg, params):
    """posetrack_train.py:155-158, on the one-launch steps of active_learning/optim.py."""
    kind = cfg.TRAIN.OPTIMIZER
    if kind == "adam":
        return optim.Adam(params, lr=cfg.TRAIN.LR)
    if kind == "rmsprop":
        return optim.RMSprop(params, lr=cfg.TRAIN.LR)
    raise ValueError(f"TRAIN.OPTIMIZER {kind!r} is not supported: 'adam' or 'rmsprop'")


# ---------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------

def epoch_batches(n: int, batch_size: int, generator=None):
    """Index lists of one epoch: a permutation from ``generator`` (None: in order), the ragged last batch kept."""
    order = torch.randperm(n, generator=generator).tolist() if generator is not None else list(range(n))
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def _collate(dataset, idxs):
    collated = getattr(dataset, "collated", None)
    if callable(collated):                                    # device-made video batches: the 11 columns directly
        return collated(idxs)
    if hasattr(dataset, "__getitems__"):
        return dataset.my_collate_fn(dataset.__getitems__(idxs))
    return dataset.my_collate_fn([dataset[i] for i in idxs])


class DecodeAhead:
    """Decodes the frames of the NEXT batch on a thread pool while the calling thread and the device work on this one.  Only for data
    sets that decode files on demand into a bounded host cache and say so (``_CocoVideo``: ``uncached_frames`` / ``cache_frames`` /
    ``reserve_frame_cache``; the eviction rule stays the data set's); anything else passes through."""

    def __init__(self, dataset, workers: int, batch_size: int = 1):
        self.dataset = dataset
        file_backed = all(callable(getattr(dataset, name, None)) for name in ("uncached_frames", "cache_frames", "reserve_frame_cache"))
        self.workers = max(0, min(int(workers), MAX_WORKERS)) if file_backed else 0
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="decode-ahead") if self.workers else None
        if self.pool is not None:                             # this batch's and the next one's frames must both fit the host cache
            dataset.reserve_frame_cache(4 * int(batch_size))
        self.futures = {}

    def submit(self, idxs):
        if self.pool is None:
            return
        from alphapose.datasets.coco_video import frame_loader
        load = frame_loader(self.dataset)                     # Pillow, or read-file + Huffman decode (the data set's DECODER)
        for path in self.dataset.uncached_frames(idxs):
            if path not in self.futures:
                self.futures[path] = self.pool.submit(load, path)

    def collect(self):
        """Hand the decoded frames to the data set's cache (on the calling thread: the cache is not shared with the pool; with device
        decoding this is where the batch's coefficient frames become pixels, in one call)."""
        if self.futures:
            self.dataset.cache_frames({path: fut.result() for path, fut in self.futures.items()})
        self.futures = {}

    def batches(self, index_lists):
        index_lists = list(index_lists)
        for k, idxs in enumerate(index_lists):
            self.collect()
            batch = _collate(self.dataset, idxs)              # enqueues this batch's crops / targets
            if k + 1 < len(index_lists):
                self.submit(index_lists[k + 1])
            yield batch

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
        self.futures = {}


# ---------------------------------------------------------------------------------------------------------------------
# one epoch, one validation pass
# ---------------------------------------------------------------------------------------------------------------------

def _device_of(model):
    p = next(model.parameters())
    if not p.is_cuda:
        raise vh.VatlError("the pose networks train on MI355X only (no CPU fallback): move the model to a HIP device")
    return p.device


def _columns(batch):
    """(inputs (B,3,H,W), labels, masks) of a data-set batch: the video 11-tuple (``inps[:, 0]``, :41-42) or the image 5-tuple."""
    if len(batch) == 11:
        return batch[1][:, 0], batch[2], batch[3]
    return batch[0], batch[1], batch[2]


def train_epoch(model, batches, optimizer, precision="fp32"):
    """``train()`` (:30-87) over any iterable of the data set's batches -> (loss, accuracy), batch-size weighted averages.
    ``precision`` "bf16" takes the bf16 trainer (same interface); the default never imports it."""
    from alphapose.models import hip_train
    if precision not in PRECISIONS:
        raise ValueError(f"TRAIN.PRECISION must be one of {sorted(PRECISIONS)}, got {precision!r}")
    device = _device_of(model)
    loss_logger, acc_logger = DataLogger(), DataLogger()
    model.train()
    if precision == "bf16":                                   # opt-in: bf16 storage and products, fp32 gradients into the same arena
        from alphapose.models import hip_train_h16
        trainer = hip_train_h16.trainer_for_h16(model)
    else:
        trainer = hip_train.trainer_for(model)
    arena = hip_train.arena_for(model)
    pending = []

    def flush():
        for loss, acc_finish, cnt in pending:
            loss_logger.update(float(loss), cnt)
            acc_logger.update(acc_finish(), cnt)
        pending.clear()
    for batch in batches:
        inps, labels, masks = _columns(batch)
        x = vh.upload(inps, device, torch.float32).contiguous()
        lab, msk = vh.upload(labels, device, torch.float32).contiguous(), vh.upload(masks, device, torch.float32)
        with torch.no_grad():
            out = trainer.forward(x)
            loss, dout = vh.masked_mse_fwd_bwd(out, lab, msk)          # 0.5 * MSE(out*m, label*m) and its gradient (:52)
            arena.begin()
            trainer.backward(dout, arena=arena)
            arena.finish()
            arena.attach()
            m = msk.reshape(msk.shape[0], -1, 1, 1)
            pending.append((loss, calc_accuracy_begin(out * m, lab * m), int(x.shape[0])))
        optimizer.step()
        if len(pending) >= FLUSH_EVERY:
            flush()
    flush()
    return loss_logger.avg, acc_logger.avg


def validate(model, cfg, dataset, work_dir, batches=None, flip_test=None):
    """``validate_gt`` (:89-133) over ``dataset`` (or over ``batches``, any iterable of its batches) ->
    {"metric", "val_metric", "records", "detail"}; writes ``<work_dir>/predicted_kpt.json``.  ``flip_test``: the ``--flip-test`` flag; None
    reads ``cfg.VAL.FLIP_TEST`` (absent: off)."""
    from active_learning.ActiveLearning import flip_test as val_flip_test
    from alphapose.models import hip_engine
    flip = val_flip_test(cfg, flip_test)                      # refused before the device is touched
    if flip:
        from alphapose.models import hip_engine_flip
    from alphapose.utils.bbox import bbox_xyxy_to_xywh
    device = _device_of(model)
    eval_joints = list(dataset.EVAL_JOINTS)
    if batches is None:
        batches = (_collate(dataset, idxs) for idxs in epoch_batches(len(dataset), int(cfg.VAL.BATCH_SIZE)))
    model.eval()                                              # the plan is keyed on the version counters the optimiser and the BN statistics bumped
    rows, oks_all = [], []
    for batch in batches:
        if len(batch) != 11:
            raise ValueError(f"validation needs a video data set ({type(dataset).__name__} yields {len(batch)}-tuples): image ids, "
                             "annotation ids and boxes come from the 11-tuple of Posetrack21 / JRDB2022 / FrameVideo items")
        _, inps, _l, _m, gt_kpts, img_ids, ann_ids, bboxes, bboxes_ann, _p, _n = batch
        x = vh.upload(inps[:, 0], device, torch.float32).contiguous()
        hm = torch.empty((x.shape[0], int(cfg.DATA_PRESET.NUM_JOINTS), *cfg.DATA_PRESET.HEATMAP_SIZE), device=device)
        with torch.no_grad():
            if flip:                                          # shift=True as in AlphaPose's validation
                hip_engine_flip.flip_forward_into(model, x, hm, dataset.joint_pairs, shift=True)
            else:
                hip_engine.forward_into(model, x, hm)
        pred = hm[:, eval_joints].contiguous()
        bb = vh.upload(bboxes, device, torch.float32).contiguous()
        coords, maxv, _ = vh.decode(pred, bb)                 # heatmap_to_coord_simple's kernel, a batch at a time
        kp = torch.cat([coords, maxv.unsqueeze(-1)], 2)
        if kp.shape[1] == 17:
            ann_xywh = bbox_xyxy_to_xywh(np.asarray(torch.as_tensor(bboxes_ann).cpu(), np.float64))
            gt = np.asarray(torch.as_tensor(gt_kpts).cpu(), np.float64).reshape(x.shape[0], -1)
            oks_all.append(vh.oks(kp.contiguous(), vh.upload(gt, device), vh.upload(np.asarray(ann_xywh, np.float64).reshape(-1, 4), device)))
        rows.append((kp, bb, list(img_ids), list(ann_ids)))
    kpt_json = []
    for kp, bb, img_ids, ann_ids in rows:                     # the read-backs, after every batch is enqueued
        kp_h, bb_h = kp.cpu().numpy(), bb.cpu().numpy()
        for j in range(kp_h.shape[0]):
            scores = kp_h[j, :, 2:3]
            kpt_json.append({"bbox": bb_h[j].tolist(), "image_id": int(img_ids[j]), "ann_id": int(ann_ids[j]),
                             "score": float(np.mean(scores) + 1.25 * np.max(scores)), "category_id": 1,
                             "keypoints": kp_h[j].reshape(-1).tolist()})
    os.makedirs(work_dir, exist_ok=True)
    res_file = os.path.join(work_dir, "predicted_kpt.json")
    with open(res_file, "w") as fid:
        json.dump(kpt_json, fid)
    if have_coco_tools():
        detail = evaluate_mAP(res_file, ann_type="keypoints", ann_file=os.path.join(cfg.DATASET.VAL.ROOT, cfg.DATASET.VAL.ANN))
        name, metric = "mAP", float(detail["AP"])
    else:
        if not oks_all:
            raise NotImplementedError("validation without the COCO API needs 17-joint key-points (vatl_oks)")
        oks = torch.cat(oks_all).cpu().numpy()
        name, metric, detail = "mOKS", float(100.0 * oks.mean()), None
    hip_engine.verify(model)
    return {"metric": metric, "val_metric": name, "records": len(kpt_json), "detail": detail}


# ---------------------------------------------------------------------------------------------------------------------
# the epoch loop
# ---------------------------------------------------------------------------------------------------------------------

def run_epochs(cfg, model, optimizer, train_fn, validate_fn, work_dir, snapshot=2, max_epochs=None, log=print, save=None, precision="fp32"):
    """posetrack_train.py:160-212 with the training epoch and the validation pass as callables: ``train_fn(epoch) -> (loss, acc)``,
    ``validate_fn(epoch) -> {"metric", "val_metric", ...}``.  Returns the run's summary dict; ``precision`` (what ``train_fn`` trains
    in) is only noted there."""
    save = save or (lambda m, path: torch.save(cpu_state_dict(m), path))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(cfg.TRAIN.LR_STEP), gamma=cfg.TRAIN.LR_FACTOR)
    out = {"work_dir": work_dir, "epochs": [], "lr": [], "train_loss": [], "train_acc": [], "val": [], "val_metric": None, "best_score": 0,
           "best_epoch": None, "saved": [], "ended": "end_epoch", "precision": precision}

    def keep(name):
        path = os.path.join(work_dir, name)
        save(model, path)
        out["saved"].append(name)
        return path
    for i in range(cfg.TRAIN.BEGIN_EPOCH, cfg.TRAIN.END_EPOCH):
        if max_epochs is not None and len(out["epochs"]) >= max_epochs:
            out["ended"] = "max_epochs"
            log(f"Stopping after {max_epochs} epoch(s) of this run (--max-epochs)")
            break
        current_lr = optimizer.param_groups[0]["lr"]
        log(f"epoch {i} starts, lr {current_lr}")
        loss, acc = train_fn(i)
        log(epoch_info("Train", i, loss, acc))
        out["epochs"].append(i); out["lr"].append(current_lr); out["train_loss"].append(loss); out["train_acc"].append(acc)
        scheduler.step()
        if snapshot and (i + 1) % snapshot == 0:
            keep("model_{}.pth".format(i))
            res = validate_fn(i)
            out["val"].append((i, res["metric"]))
            out["val_metric"] = res["val_metric"]
            log(f"epoch {i} validation, {res['val_metric']} {res['metric']}")
            if res["metric"] > out["best_score"]:
                out["best_score"], out["best_epoch"] = res["metric"], i
                log(f"Best score so far: saved {keep('model_best.pth')}")
        if i == cfg.TRAIN.DPG_MILESTONE:
            keep("final.pth")
            for param_group in optimizer.param_groups:
                param_group["lr"] = cfg.TRAIN.LR
            scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(cfg.TRAIN.DPG_STEP), gamma=0.1)
            out["ended"] = "dpg_milestone"
            log(f"DPG milestone (epoch {i}): final.pth saved, lr reset to {cfg.TRAIN.LR}; the DPG stage has no data set here, training ends")
            break
    out["final_lr"] = optimizer.param_groups[0]["lr"]
    return out


def seed_everything(seed: int):
    torch.manual_seed(seed)
    np.random.seed(seed % (2 ** 32))
    random.seed(seed)


def main(argv=None):
    opt = parse_args(argv)
    cfg = load_config(opt.cfg)
    precision = train_precision(cfg, opt.precision)           # refused here: before the device, the work dir and the data sets
    from active_learning.ActiveLearning import flip_test
    flip = flip_test(cfg, True if opt.flip_test else None)    # ... and so is a bad VAL.FLIP_TEST
    if not torch.cuda.is_available():
        raise vh.VatlError("the pose networks train on MI355X only (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    work_dir = work_dir_for(opt.exp_id, cfg)
    logger = make_logger(work_dir)
    log = logger.info
    pool = None
    try:
        log(f"options: {vars(opt)}")
        log(f"config: {dict(cfg)}")
        log(f"training precision: {precision} (TRAIN.PRECISION / --precision; checkpoints and validation are fp32)")
        seed_everything(opt.seed)
        if opt.validate_only:
            cfg.MODEL.PRETRAINED, cfg.MODEL.TRY_LOAD = opt.validate_only, ""
        model = preset_model(cfg, log=log).to(device)
        val_set = builder.build_dataset(cfg.DATASET.VAL, preset_cfg=cfg.DATA_PRESET, train=False)
        if hasattr(val_set, "emit_neighbour_crops"):
            val_set.emit_neighbour_crops = False              # only inps[:, 0] is read
        if opt.validate_only:
            res = validate(model, cfg, val_set, work_dir, flip_test=flip)
            log(f"{opt.validate_only} validation, {res['val_metric']} {res['metric']}")
            return {"work_dir": work_dir, "val": [(None, res["metric"])], "val_metric": res["val_metric"], "ended": "validate_only"}
        optimizer = build_optimizer(cfg, model.parameters())
        train_set = builder.build_dataset(cfg.DATASET.TRAIN, preset_cfg=cfg.DATA_PRESET, train=True)
        if hasattr(train_set, "emit_neighbour_crops"):
            train_set.emit_neighbour_crops = False
        batch_size = int(cfg.TRAIN.BATCH_SIZE)
        pool = DecodeAhead(train_set, opt.workers, batch_size)
        gen = torch.Generator()
        gen.manual_seed(opt.seed)
        log(f"train items: {len(train_set)}, validation items: {len(val_set)}, decode-ahead threads: {pool.workers}")
        out = run_epochs(cfg, model, optimizer,
                         train_fn=lambda i: train_epoch(model, pool.batches(epoch_batches(len(train_set), batch_size, gen)), optimizer, precision),
                         validate_fn=lambda i: validate(model, cfg, val_set, work_dir, flip_test=flip),
                         work_dir=work_dir, snapshot=opt.snapshot, max_epochs=opt.max_epochs, log=log, precision=precision)
        log(f"run ended: {out['ended']}; best {out['val_metric']}: {out['best_score']} (epoch {out['best_epoch']})")
        out["model"] = model
        return out
    finally:
        if pool is not None:
            pool.close()
        close_logger(logger)


if __name__ == "__main__":
    main()
