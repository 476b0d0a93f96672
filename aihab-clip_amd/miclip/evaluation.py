"""Validation metrics on the GPU: loss, top-k, F1, MCC, confusion, L2 roll-up.

Counterpart of `_run_validation` (methods/PEFT_openclip.py:50-136) and of
aihab_utils/evaluation.py (same names, keyword signatures and return shapes):
`run_validation`, `map_l3_targets_to_l2`, `aggregate_logits_to_l2`,
`L2MetricsAccumulator` and `ClassificationTracker`, plus `evaluate_features`, the
same evaluation over already-encoded features (the embeddings cache, or the output
of ProLIP's projector), and `Evaluator`, the object all of them drive.

Per batch there is one call, miclip_eval_batch (csrc/evaluate.hip): normalise,
`scale * f @ W`, cross-entropy, top-3 with softmax probabilities, the L3 -> L2
roll-up and every counter update, accumulated in a device state block. The
reference runs about a dozen torch ops per batch with an `.item()` each; here
nothing synchronises until the state block is read, once, at the end. Weighted F1
and MCC are derived on the host in float64 from the exact integer confusion counts:
F1 is torcheval's weighted MulticlassF1Score (= sklearn's f1_score(average=
"weighted", zero_division=0)), MCC is sklearn.metrics.matthews_corrcoef's
multiclass formula.

Departures from the reference:
  * W&B logging and `draw_cm` (:14-77) are out of scope: they are plots on top of the
    confusion matrix that `run_validation(return_confusion_matrix=True)` returns.
    `ClassificationTracker.save_classification(out_dir)` writes two CSV files
    instead of two W&B tables; `frames()` returns the same two tables;
  * `class_names` replaces the dataset constant REASSIGN_LABEL_NAME_L3;
  * L2 top-k is available for k = 1 and k = 3 (the kernel keeps three picks);
  * a batch without metadata is tracked with empty metadata fields (the reference
    fails on `metadata['file_name']`).
There is no CPU fallback: every computing call raises RuntimeError without a device.
"""
import ctypes
import os
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .feature_cache import AsyncHostSink, _model_device, prepare_images

_F_DTYPES = {torch.float32: _lib.MICLIP_F32, torch.float16: _lib.MICLIP_FP16,
             torch.bfloat16: _lib.MICLIP_BF16}
_REDUCE = {"sum": _lib.MICLIP_EVAL_L2_SUM, "mean": _lib.MICLIP_EVAL_L2_MEAN,
           "logsumexp": _lib.MICLIP_EVAL_L2_LOGSUMEXP}
_HEADER_WORDS = 8    # include/miclip.h: the state block's layout


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _device(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError("miclip evaluation needs a HIP device (no CPU fallback)")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("miclip evaluation needs a HIP device (no CPU fallback)")
    return device


def _map_list(l3_to_l2):
    if torch.is_tensor(l3_to_l2):
        return [int(v) for v in l3_to_l2.detach().cpu().tolist()]
    return [int(v) for v in l3_to_l2]


# ------------------------------------------------------------------ host metrics
def weighted_f1(cm) -> float:
    """Weighted F1 from confusion counts (rows = true): sum_c support_c / N *
    2 TP_c / (pred_c + support_c), 0 / 0 taken as 0."""
    cm = np.asarray(cm, dtype=np.float64)
    tp, support, pred = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    n = support.sum()
    if n == 0:
        return 0.0
    den = pred + support
    f1 = np.divide(2.0 * tp, den, out=np.zeros_like(den), where=den > 0)
    return float((f1 * support).sum() / n)


def mcc_from_confusion(cm) -> float:
    """sklearn.metrics.matthews_corrcoef's multiclass formula on confusion counts."""
    cm = np.asarray(cm, dtype=np.float64)
    t_sum, p_sum = cm.sum(axis=1), cm.sum(axis=0)
    n_correct, n = np.trace(cm), p_sum.sum()
    cov_ytyp = n_correct * n - np.dot(t_sum, p_sum)
    cov_ypyp = n ** 2 - np.dot(p_sum, p_sum)
    cov_ytyt = n ** 2 - np.dot(t_sum, t_sum)
    if cov_ypyp * cov_ytyt == 0:
        return 0.0
    return float(cov_ytyp / np.sqrt(cov_ytyt * cov_ypyp))


class EvalCounts:
    """The state block on the host (one copy): loss_sum float64, the integer counters
    and the two confusion matrices (int64, rows = true labels)."""

    def __init__(self, words: np.ndarray, C: int, num_l2: int):
        self.loss_sum = float(words[:1].view(np.float64)[0])
        (self.rows, self.batches, self.top1, self.top3, self.l2_top1, self.l2_top3,
         self.skipped) = (int(v) for v in words[1:_HEADER_WORDS])
        self.cm = words[_HEADER_WORDS:_HEADER_WORDS + C * C].reshape(C, C).copy()
        self.cm_l2 = words[_HEADER_WORDS + C * C:].reshape(num_l2, num_l2).copy()


# ------------------------------------------------------------------ the kernel's driver
class Evaluator:
    """Accumulates the metrics of `scale * normalize(feats) @ text_weights` against
    labels, one miclip_eval_batch call per `update`.

    l2_eval_ctx: the reference's dict {"l3_to_l2", "num_l2", "reduce" ("mean"),
    "topk" ((1, 3)), "mode" ("argmax"), "return_confusion_matrix" (False)}.
    `update` returns the batch's per-row device tensors; `counts()` reads the state
    block (the only synchronising call); `compute()` returns the reference's 7-tuple.
    """

    def __init__(self, text_weights=None, *, num_classes: Optional[int] = None,
                 scale: float = 100.0, l2_eval_ctx: Optional[Dict] = None, device=None):
        self.device = _device(device)
        if text_weights is not None:
            if not isinstance(text_weights, torch.Tensor) or text_weights.ndim != 2 or \
                    not text_weights.is_floating_point():
                raise ValueError("Expected text_weights as a floating [E, C] tensor.")
            self.E, self.C = (int(s) for s in text_weights.shape)
            if self.E % 16 or not 16 <= self.E <= 1024:
                raise ValueError(f"unsupported E={self.E}: need E % 16 == 0 in [16, 1024].")
        else:
            if num_classes is None:
                raise ValueError("text_weights or num_classes is required.")
            self.E, self.C = 0, int(num_classes)
        if not 3 <= self.C <= 1024:
            raise ValueError(f"unsupported C={self.C}: need 3 <= C <= 1024 (topk(3) needs 3 classes).")
        self.scale = float(scale)
        self.l2_mode, self.num_l2, self._map, self.l2_ctx = _lib.MICLIP_EVAL_L2_NONE, 1, None, None
        if l2_eval_ctx is not None:
            ctx = dict(l2_eval_ctx)
            mode, reduce = ctx.get("mode", "argmax"), ctx.get("reduce", "mean")
            if mode not in {"argmax", "logits"}:
                raise ValueError(f"Unsupported mode='{mode}'. Expected 'argmax' or 'logits'.")
            if reduce not in _REDUCE:
                raise ValueError(f"Unsupported reduce='{reduce}'. Expected one of: sum, mean, logsumexp.")
            m = _map_list(ctx["l3_to_l2"])
            self.num_l2 = int(ctx["num_l2"])
            if len(m) != self.C:
                raise ValueError(f"logits_l3 has {self.C} classes, but l3_to_l2 has {len(m)} entries.")
            if not 1 <= self.num_l2 <= self.C:
                raise ValueError(f"num_l2 must lie in [1, {self.C}], got {self.num_l2}.")
            if min(m) < 0 or max(m) >= self.num_l2:
                raise ValueError(f"l3_to_l2 entries must lie in [0, {self.num_l2}); got "
                                 f"[{min(m)}, {max(m)}].")
            self._map = np.ascontiguousarray(m, dtype=np.int32)
            self.l2_mode = _lib.MICLIP_EVAL_L2_ARGMAX if mode == "argmax" else _REDUCE[reduce]
            topk = (1,) if mode == "argmax" else tuple(int(k) for k in ctx.get("topk", (1, 3)))
            for k in topk:
                if min(k, self.num_l2) not in (1, min(3, self.num_l2)) and k >= 1:
                    raise ValueError(f"L2 topk={k} is not supported: the kernel keeps 3 picks.")
            self.l2_ctx = {"mode": mode, "reduce": reduce, "topk": topk,
                           "return_confusion_matrix": bool(ctx.get("return_confusion_matrix", False))}
        self.lib = _lib.load_library()
        self.tw = None if text_weights is None else \
            text_weights.detach().to(self.device, torch.float32).contiguous()
        words = int(self.lib.miclip_eval_state_bytes(self.C, self.num_l2)) // 8
        if words < _HEADER_WORDS:
            raise ValueError(f"unsupported C={self.C}, num_l2={self.num_l2}.")
        self.state = torch.empty(words, dtype=torch.int64, device=self.device)
        self.reset()

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self.lib.miclip_eval_reset(_ptr(self.state), self.C, self.num_l2,
                                                  _lib.stream_handle(self.device)),
                       "miclip_eval_reset")

    def _labels(self, labels, B):
        if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] != B:
            raise ValueError(f"Expected labels shape [{B}], got {tuple(getattr(labels, 'shape', ()))}.")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError(f"Expected integer labels, got dtype={labels.dtype}.")
        if not labels.is_cuda and B:   # host labels: checked here; device labels: the skipped word
            lo, hi = int(labels.min()), int(labels.max())
            if lo < 0 or hi >= self.C:
                raise ValueError(f"labels must lie in [0, {self.C}); got [{lo}, {hi}].")
        return labels.detach().to(self.device, torch.int64, non_blocking=True).contiguous()

    def _run(self, feats, logits_in, labels, rows, want_logits, want_l2_logits):
        B, dev, i32, f32 = int(labels.shape[0]), self.device, torch.int32, torch.float32
        agg = self.l2_mode >= _lib.MICLIP_EVAL_L2_SUM
        out = {"row_loss": torch.empty(B, device=dev, dtype=f32)}
        if rows:
            out["pred"] = torch.empty(B, device=dev, dtype=i32)
            out["top3"] = torch.empty(B, 3, device=dev, dtype=i32)
            out["top3_prob"] = torch.empty(B, 3, device=dev, dtype=f32)
            if self.l2_mode:
                out["l2_pred"] = torch.empty(B, device=dev, dtype=i32)
                out["l2_top3"] = torch.empty(B, 3, device=dev, dtype=i32)
        if logits_in is not None:
            out["logits"] = logits_in
        elif want_logits:
            out["logits"] = torch.empty(B, self.C, device=dev, dtype=f32)
        if want_l2_logits and agg:
            out["l2_logits"] = torch.empty(B, self.num_l2, device=dev, dtype=f32)
        with torch.cuda.device(dev):
            _lib.check(self.lib.miclip_eval_batch(
                _ptr(feats), _F_DTYPES[feats.dtype] if feats is not None else _lib.MICLIP_F32,
                _ptr(self.tw), _ptr(labels), B, self.E, self.C, self.scale,
                self._map.ctypes.data_as(ctypes.c_void_p) if self._map is not None else None,
                self.num_l2, self.l2_mode,
                _lib.MICLIP_EVAL_LOGITS_IN if logits_in is not None else 0, _ptr(self.state),
                _ptr(out.get("logits")), _ptr(out["row_loss"]), _ptr(out.get("pred")),
                _ptr(out.get("top3")), _ptr(out.get("top3_prob")), _ptr(out.get("l2_pred")),
                _ptr(out.get("l2_top3")), _ptr(out.get("l2_logits")),
                _lib.stream_handle(dev)), "miclip_eval_batch")
        return out

    def update(self, feats, labels, *, rows: bool = False, want_logits: bool = False,
               want_l2_logits: bool = False):
        """One batch of features [B, E] (fp32, fp16 or bf16) and labels [B]."""
        if self.tw is None:
            raise ValueError("this Evaluator was built without text_weights: use update_logits.")
        if not isinstance(feats, torch.Tensor) or feats.ndim != 2 or feats.shape[1] != self.E:
            raise ValueError(f"Expected feats shape [B, {self.E}], got "
                             f"{tuple(getattr(feats, 'shape', ()))}.")
        if feats.dtype not in _F_DTYPES:
            raise TypeError(f"Expected feats dtype float32, float16 or bfloat16, got {feats.dtype}.")
        if feats.shape[0] < 1:
            raise ValueError("Empty inputs: feats has no rows.")
        y = self._labels(labels, int(feats.shape[0]))
        f = feats.detach().to(self.device, non_blocking=True).contiguous()
        return self._run(f, None, y, rows, want_logits, want_l2_logits)

    def update_logits(self, logits, labels, *, rows: bool = False, want_l2_logits: bool = False):
        """One batch of ready logits [B, C] (the form of L2MetricsAccumulator.update)."""
        if not isinstance(logits, torch.Tensor) or logits.ndim != 2 or logits.shape[1] != self.C:
            raise ValueError(f"Expected logits shape [B, {self.C}], got "
                             f"{tuple(getattr(logits, 'shape', ()))}.")
        if logits.shape[0] < 1:
            raise ValueError("Empty inputs: logits has no rows.")
        y = self._labels(labels, int(logits.shape[0]))
        lg = logits.detach().to(self.device, torch.float32).contiguous()
        return self._run(None, lg, y, rows, False, want_l2_logits)

    def counts(self) -> EvalCounts:
        return EvalCounts(self.state.cpu().numpy(), self.C, self.num_l2)

    def l2_metrics(self, c: EvalCounts) -> Optional[dict]:
        """The dict of L2MetricsAccumulator.compute (evaluation.py:223-250)."""
        if self.l2_ctx is None:
            return None
        metrics, denom = {}, max(c.rows, 1)
        for k in self.l2_ctx["topk"]:
            metrics[f"top{k}"] = (c.l2_top1 if min(k, self.num_l2) == 1 else c.l2_top3) / denom
        want_cm = self.l2_ctx["return_confusion_matrix"]
        if c.rows == 0:
            metrics.update(f1=0.0, mcc=0.0,
                           cm=np.zeros((self.num_l2, self.num_l2)) if want_cm else None)
            return metrics
        metrics.update(f1=weighted_f1(c.cm_l2), mcc=mcc_from_confusion(c.cm_l2),
                       cm=c.cm_l2 if want_cm else None)
        return metrics

    def compute(self, return_confusion_matrix: bool = False):
        """(avg_loss, avg_top1, avg_top3, f1_weighted, mcc, confusion_matrix | None,
        l2_metrics | None), PEFT_openclip.py:119-136. One device read."""
        c = self.counts()
        if c.skipped:
            raise ValueError(f"{c.skipped} rows had a label outside [0, {self.C}) or NaN logits.")
        return (c.loss_sum / max(c.batches, 1), c.top1 / max(c.rows, 1), c.top3 / max(c.rows, 1),
                weighted_f1(c.cm), mcc_from_confusion(c.cm),
                c.cm if return_confusion_matrix else None, self.l2_metrics(c))


# ------------------------------------------------------------------ aihab_utils/evaluation.py
def map_l3_targets_to_l2(targets_l3: torch.Tensor,
                         l3_to_l2: Union[Sequence[int], torch.Tensor]) -> torch.Tensor:
    """L3 target indices -> L2 indices through a lookup vector (evaluation.py:80-89)."""
    lut = torch.as_tensor(l3_to_l2 if torch.is_tensor(l3_to_l2) else list(l3_to_l2))
    return lut.to(device=targets_l3.device, dtype=torch.long)[targets_l3.long()]


def aggregate_logits_to_l2(logits_l3: torch.Tensor, l3_to_l2: Union[Sequence[int], torch.Tensor],
                           num_l2: int, reduce: str = "mean") -> torch.Tensor:
    """L3 logits [B, C] -> L2 logits [B, num_l2] per group by sum / mean / logsumexp in
    ascending L3 id (evaluation.py:92-142), in the evaluation kernel."""
    dev = _device(logits_l3.device if isinstance(logits_l3, torch.Tensor) and logits_l3.is_cuda
                  else None)
    m = _map_list(l3_to_l2)
    if int(logits_l3.shape[1]) != len(m):
        raise ValueError(
            f"logits_l3 has {int(logits_l3.shape[1])} classes, but l3_to_l2 has {len(m)} entries.")
    if reduce not in _REDUCE:
        raise ValueError(f"Unsupported reduce='{reduce}'. Expected one of: sum, mean, logsumexp.")
    B = int(logits_l3.shape[0])
    if B == 0:
        return torch.zeros(0, int(num_l2), device=logits_l3.device, dtype=logits_l3.dtype)
    ev = Evaluator(num_classes=len(m), device=dev,
                   l2_eval_ctx={"l3_to_l2": m, "num_l2": num_l2, "reduce": reduce, "mode": "logits"})
    out = ev.update_logits(logits_l3, torch.zeros(B, dtype=torch.int64), want_l2_logits=True)
    return out["l2_logits"].to(device=logits_l3.device, dtype=logits_l3.dtype)


class L2MetricsAccumulator:
    """L2 metrics from L3 logits / targets through a fixed L3 -> L2 map
    (evaluation.py:145-250): top-k accuracy, weighted F1, MCC and optionally the
    confusion matrix. Mode "argmax" maps the L3 argmax to L2 and reports top-1 only;
    mode "logits" aggregates the logits per group and supports top-k."""

    def __init__(self, l3_to_l2: Union[Sequence[int], torch.Tensor], num_l2: int,
                 reduce: str = "mean", topk: Sequence[int] = (1, 3),
                 return_confusion_matrix: bool = False, mode: str = "argmax") -> None:
        if mode not in {"argmax", "logits"}:
            raise ValueError(f"Unsupported mode='{mode}'. Expected 'argmax' or 'logits'.")
        self.l3_to_l2, self.num_l2 = l3_to_l2, int(num_l2)
        self.reduce, self.mode = reduce, mode
        # mode argmax reports top-1 only, whatever topk says
        self.topk = (1,) if mode == "argmax" else tuple(int(k) for k in topk)
        self.return_confusion_matrix = return_confusion_matrix
        self.total_seen = 0
        self._ev = None

    def _ctx(self):
        return {"l3_to_l2": self.l3_to_l2, "num_l2": self.num_l2, "reduce": self.reduce,
                "topk": self.topk, "mode": self.mode,
                "return_confusion_matrix": self.return_confusion_matrix}

    def update(self, logits_l3: torch.Tensor, targets_l3: torch.Tensor) -> None:
        """One batch of L3 logits [B, C] and L3 targets [B]."""
        dev = _device(logits_l3.device if logits_l3.is_cuda else None)
        batch_size = int(targets_l3.shape[0])
        self.total_seen += batch_size
        if batch_size == 0:
            return
        if self._ev is None:
            self._ev = Evaluator(num_classes=int(logits_l3.shape[1]), l2_eval_ctx=self._ctx(),
                                 device=dev)
        self._ev.update_logits(logits_l3, targets_l3)

    def compute(self) -> dict:
        if self._ev is None:
            _device()
            metrics = {f"top{k}": 0.0 for k in self.topk}
            metrics.update(f1=0.0, mcc=0.0, cm=np.zeros((self.num_l2, self.num_l2))
                           if self.return_confusion_matrix else None)
            return metrics
        c = self._ev.counts()
        if c.skipped:
            raise ValueError(f"{c.skipped} rows had a target outside [0, {self._ev.C}).")
        return self._ev.l2_metrics(c)


TRACK_COLUMNS = ("file_name", "ground_truth_num_label", "ground_truth_word_label",
                 "predicted_label", "predicted_word_label", "dataset", "top3_label_1",
                 "top3_prob_1", "top3_label_2", "top3_prob_2", "top3_label_3", "top3_prob_3")


class ClassificationTracker:
    """Per-sample table of the prediction and the top-3 labels with their softmax
    probabilities, split into misclassified and correctly classified samples
    (evaluation.py:253-347)."""

    def __init__(self, class_names: Optional[Sequence[str]] = None) -> None:
        self.class_names = list(class_names) if class_names is not None else None
        self.misclassified = []
        self.accurate_classified = []

    def top3_metrics(self, outputs, labels):
        """(top3_correct, top3_pred_indices [B, 3], top3_probs [B, 3]) of logits, :261-273."""
        dev = _device(outputs.device if outputs.is_cuda else None)
        ev = Evaluator(num_classes=int(outputs.shape[1]), device=dev)
        out = ev.update_logits(outputs, labels, rows=True)
        idx = out["top3"].long()
        correct = torch.sum(torch.any(idx == labels.to(idx.device).unsqueeze(1), dim=1))
        return correct, idx, out["top3_prob"]

    def _word(self, p):
        if self.class_names is not None and 0 <= p < len(self.class_names):
            return self.class_names[p]
        return str(p)

    def track_classification(self, predictions, labels, top3_labels, top3_probs, metadata):
        """Append one row per sample (:275-301). Arguments are host or device arrays."""
        def host(t):
            return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        predictions, labels = host(predictions), host(labels)
        top3_labels, top3_probs = host(top3_labels), host(top3_probs)
        meta = metadata if isinstance(metadata, dict) else {}

        def field(key, i):
            v = meta.get(key)
            if v is None:
                return None
            v = v[i]
            return v.item() if isinstance(v, (torch.Tensor, np.generic)) else v
        for i in range(len(labels)):
            pred = int(predictions[i])
            row = {
                "file_name": field("file_name", i),
                "ground_truth_num_label": int(labels[i]),
                "ground_truth_word_label": field("plot_word_label", i),
                "predicted_label": pred,
                "predicted_word_label": self._word(pred),
                "top3_predictions": [{"label": int(top3_labels[i][j]),
                                      "probability": float(top3_probs[i][j])} for j in range(3)],
                "dataset": field("image_source", i),
            }
            (self.misclassified if pred != int(labels[i]) else self.accurate_classified).append(row)

    @staticmethod
    def _flatten(instance_results):
        import pandas as pd
        flat = []
        for inst in instance_results:
            base = {k: inst[k] for k in TRACK_COLUMNS[:6]}
            for i, e in enumerate(inst["top3_predictions"]):
                base[f"top3_label_{i + 1}"] = e["label"]
                base[f"top3_prob_{i + 1}"] = e["probability"]
            flat.append(base)
        return pd.DataFrame(flat, columns=list(TRACK_COLUMNS))

    def frames(self):
        """(misclassified_df, correct_df) with the reference's flattened columns (:309-335)."""
        return self._flatten(self.misclassified), self._flatten(self.accurate_classified)

    def save_classification(self, out_dir=None):
        """Write misclassified.csv / correct.csv into out_dir (the reference logs the
        two tables to W&B); prints the reference's lines for an empty table."""
        mis_df, cor_df = self.frames()
        for rows, df, name, empty in (
                (self.misclassified, mis_df, "misclassified.csv", "No misclassified samples"),
                (self.accurate_classified, cor_df, "correct.csv", "No correctly classified samples")):
            if not rows:
                print(empty)
            elif out_dir is not None:
                os.makedirs(out_dir, exist_ok=True)
                df.to_csv(os.path.join(out_dir, name), index=False)


# ------------------------------------------------------------------ the two entry points
class _RowSink:
    """The kernel's per-row outputs of every batch, copied to the host asynchronously."""

    def __init__(self):
        self.ints, self.probs, self.labels, self.meta = AsyncHostSink(), AsyncHostSink(), [], []

    def push(self, out, labels, metadata):
        self.ints.push(torch.cat([out["pred"][:, None], out["top3"]], dim=1))
        self.probs.push(out["top3_prob"])
        self.labels.append(labels.detach().to("cpu"))
        self.meta.append(metadata)

    def fill(self, tracker: ClassificationTracker):
        ints, probs = self.ints.result().numpy(), self.probs.result().numpy()
        i0 = 0
        for labels, metadata in zip(self.labels, self.meta):
            i1 = i0 + len(labels)
            tracker.track_classification(ints[i0:i1, 0], labels, ints[i0:i1, 1:], probs[i0:i1],
                                         metadata)
            i0 = i1


def _tracker(cls_track, class_names):
    if isinstance(cls_track, ClassificationTracker):
        if class_names is not None:
            cls_track.class_names = list(class_names)
        return cls_track
    return ClassificationTracker(class_names)


@torch.no_grad()
def run_validation(model, loader, text_weights, device=None, return_confusion_matrix: bool = False,
                   cls_track: bool = False, l2_eval_ctx: Optional[Dict] = None, class_names=None):
    """`_run_validation` (methods/PEFT_openclip.py:50-136): returns (avg_loss, avg_top1,
    avg_top3, f1_weighted, mcc, confusion_matrix | None, l2_metrics | None); the two
    accuracies are fractions. Batches are (images, targets) or (images, targets,
    metadata). cls_track may be a ClassificationTracker to fill (True fills an internal
    one, whose tables the reference would log to W&B); class_names names its
    predictions."""
    dev = _device(device if device is not None else
                  (_model_device(model) if torch.cuda.is_available() else None))
    if hasattr(model, "eval"):
        model.eval()
    ev = Evaluator(text_weights, l2_eval_ctx=l2_eval_ctx, device=dev)
    sink = _RowSink() if cls_track else None
    for batch in loader:
        if isinstance(batch, (list, tuple)) and len(batch) == 3:
            images, targets, metadata = batch
        elif isinstance(batch, (list, tuple)) and len(batch) == 2:
            images, targets = batch
            metadata = None
        else:
            raise ValueError("Expected batch to be (images, targets) or (images, targets, metadata).")
        feats = model.encode_image(prepare_images(model, images, dev))
        out = ev.update(feats, targets, rows=bool(cls_track))
        if sink is not None:
            sink.push(out, targets, metadata)
    result = ev.compute(return_confusion_matrix)
    if sink is not None:
        tracker = _tracker(cls_track, class_names)
        sink.fill(tracker)
        tracker.save_classification()
    return result


@torch.no_grad()
def evaluate_features(feats, labels, text_weights, *, batch_size: int = 0, scale: float = 100.0,
                      return_confusion_matrix: bool = False, cls_track: bool = False,
                      l2_eval_ctx: Optional[Dict] = None, class_names=None, metadata=None,
                      device=None):
    """run_validation over already-encoded features [N, E] (fp32 / fp16 / bf16) and
    labels [N]: the same 7-tuple. batch_size = 0 is one batch; otherwise rows are taken
    in order in batches of batch_size (the loss is the mean of the batch means, as in
    the reference). cls_track is True or a ClassificationTracker to fill; metadata is
    the dict of per-sample lists of the reference's loader."""
    dev = _device(device if device is not None else
                  (feats.device if isinstance(feats, torch.Tensor) and feats.is_cuda else None))
    ev = Evaluator(text_weights, scale=scale, l2_eval_ctx=l2_eval_ctx, device=dev)
    if not isinstance(feats, torch.Tensor) or feats.ndim != 2:
        raise ValueError(f"Expected feats shape [N, E], got {tuple(getattr(feats, 'shape', ()))}.")
    n, bs = int(feats.shape[0]), int(batch_size or 0)
    if n < 1 or bs < 0:
        raise ValueError("Empty inputs: feats has no rows." if n < 1 else "batch_size must be >= 0.")
    y = ev._labels(labels, n)
    f = feats.detach().to(dev).contiguous()
    sink = _RowSink() if cls_track else None
    y_host = labels.detach().to("cpu") if cls_track else None
    for i0 in range(0, n, bs or n):
        i1 = min(i0 + (bs or n), n)
        out = ev.update(f[i0:i1], y[i0:i1], rows=bool(cls_track))
        if sink is not None:
            md = None if metadata is None else {k: v[i0:i1] for k, v in metadata.items()}
            sink.push(out, y_host[i0:i1], md)
    result = ev.compute(return_confusion_matrix)
    if sink is not None:
        sink.fill(_tracker(cls_track, class_names))
    return result
