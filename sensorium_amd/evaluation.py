"""Trial-level evaluation on the device: the out-of-fold and the repeat scores of the competition.

What the reference's ``evaluate_folds_predictions`` (src/submission.py:20-45) computes — cut every trial to the scored frames,
concatenate all trials of a mouse, take the per-neuron ``corr`` — and the scores that need the structure "which trials showed the
same video": correlation to the trial average, the fraction of explainable variance explained (FEVE) and the per-neuron
reliability (leave-one-out oracle correlation).  The predictions stay on the device (``Predictor.predict_trial(to_numpy=False)``);
``dwn_trial_moments`` merges the centred float64 moments of the trials added so far into a per-neuron state and
``dwn_trial_score_finalize`` turns the state into the scores and a summary that one read-back fetches.  File I/O, trial ids, tiers
and video hashes are the caller's: it supplies tensors and group ids.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Hashable, Iterable, Optional

import torch

from . import _lib as L
from . import ops


@dataclass(frozen=True)
class FrameCut:
    """The kept frames ``[skip_first, min(L, limit_length) - skip_last)`` of a trial of length ``L``: the reference's
    ``x[..., :limit_length][..., skip_first:][..., :-skip_last]`` (src/submission.py:12-17; no last slice for ``skip_last == 0``)."""
    skip_first: int = 0
    limit_length: Optional[int] = None
    skip_last: int = 0

    def __post_init__(self):
        if self.skip_first < 0 or self.skip_last < 0 or (self.limit_length is not None and self.limit_length < 0):
            raise ValueError(f"FrameCut: negative field in {self}")

    @classmethod
    def submission(cls) -> "FrameCut":
        """src/constants.py:52-54: the frames the competition scores."""
        return cls(50, 300, 1)

    def bounds(self, length: int):
        """``(start, stop)`` of the kept frames of a trial of ``length`` frames; ``ValueError`` when none is kept."""
        length = int(length)
        lim = length if self.limit_length is None else min(length, self.limit_length)
        start, stop = self.skip_first, lim - self.skip_last
        if length < 0 or stop <= start:
            raise ValueError(f"{self} keeps no frame of a trial of length {length}")
        return start, stop


SCORE_NAMES = ("single_trial_corr", "corr_to_average", "fev", "feve", "oracle_corr")


class TrialScores:
    """The five per-neuron scores of one mouse as ``[N]`` float64 device tensors (views of one ``[5, N]`` tensor) and the counts
    ``n_all`` (kept frames of all trials), ``n_repeat`` (of the trials in repeat groups) and ``n_group_frames`` (kept frames of the
    repeat groups, each counted once).  Nothing here has been read back; ``summary()`` is the one read-back."""

    def __init__(self, scores: torch.Tensor, summary: torch.Tensor, counts, fev_threshold: float):
        self.scores, self._summary = scores, summary
        self.n_all, self.n_repeat, self.n_group_frames = (int(c) for c in counts)
        self.fev_threshold = float(fev_threshold)
        for i, name in enumerate(SCORE_NAMES):
            setattr(self, name, scores[i])

    def summary(self) -> Dict[str, float]:
        """The means over all neurons of single_trial_corr, corr_to_average and oracle_corr (NaN as soon as one neuron is NaN, as
        ``corr(...).mean()`` in the reference), the mean of feve over the neurons with ``fev >= fev_threshold`` and their number,
        and the three counts: decided on the device, fetched by one copy."""
        s = self._summary.cpu().tolist()
        return {"single_trial_corr": s[0], "corr_to_average": s[1], "oracle_corr": s[2], "feve": s[3], "n_feve_neurons": int(s[4]),
                "fev_threshold": self.fev_threshold, "n_all": int(s[5]), "n_repeat": int(s[6]), "n_group_frames": int(s[7])}

    def reliable(self, min_oracle_corr: float) -> torch.Tensor:
        """The indices of the neurons with ``oracle_corr >= min_oracle_corr`` (a NaN is not) as a 1-D int64 device tensor: what the
        ``neurons=`` argument of ``attribution.input_gradient`` / ``most_exciting_input`` / ``tuning_curve`` takes as is."""
        return torch.nonzero(self.oracle_corr >= float(min_oracle_corr)).flatten()


class TrialScorer:
    """Accumulates the trials of ONE mouse and scores them (module docstring).  ``add`` keeps references to device tensors,
    ``flush`` merges them into the float64 state with one launch and drops the references, so a scorer can be flushed as often as
    memory demands; ``compute`` flushes and finalises.  Trials that carry the same ``group`` id showed the same video; a group is
    complete when it is flushed (adding to it afterwards raises), and a group id seen once counts as no group.  Flushing keeps
    the order of first appearance of the groups, and the state after several flushes equals the state after one, bit for bit."""

    def __init__(self, num_neurons: int, device, cut: FrameCut = FrameCut(), eps: float = 1e-8, fev_threshold: float = 0.15):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"sensorium_amd.TrialScorer: needs a GPU device (got {self.device}); the HIP path has no CPU fallback")
        self.num_neurons, self.cut, self.eps, self.fev_threshold = int(num_neurons), cut, float(eps), float(fev_threshold)
        if self.num_neurons < 1:
            raise ValueError("TrialScorer: num_neurons must be positive")
        self.state: Optional[torch.Tensor] = None
        self.counts = (0, 0, 0)
        self._pending: list = []                 # (group key or None, pred, target, first, frames)
        self._flushed_groups: set = set()

    def add(self, pred: torch.Tensor, target: torch.Tensor, group: Optional[Hashable] = None, length: Optional[int] = None):
        """One trial: ``pred`` and ``target`` ``[N, L]`` fp32 device tensors (unit stride along frames, any row stride; they may
        differ in ``L``, the shorter counts).  ``length`` trims the tail first (the NaN padding of a stored target)."""
        if group is not None and group in self._flushed_groups:
            raise ValueError(f"TrialScorer.add: group {group!r} was already flushed; add all trials of a group before flush()")
        for t in (pred, target):
            if t.dtype != torch.float32:
                raise RuntimeError(f"sensorium_amd.TrialScorer.add: trials must be fp32 (got {t.dtype})")
            if t.dim() != 2 or t.shape[0] != self.num_neurons:
                raise ValueError(f"TrialScorer.add: a trial is [N = {self.num_neurons}, L], got {tuple(t.shape)}")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError(f"TrialScorer.add: frames must have unit stride (got {t.stride(1)})")
        total = min(int(pred.shape[1]), int(target.shape[1]))
        if length is not None:
            if not 0 <= int(length) <= total:
                raise ValueError(f"TrialScorer.add: length {length} outside [0, {total}]")
            total = int(length)
        start, stop = self.cut.bounds(total)
        frames = stop - start
        if group is not None:
            for key, _, _, _, k in self._pending:
                if key == group and k != frames:
                    raise ValueError(f"TrialScorer.add: group {group!r} keeps {k} frames per trial, this trial keeps {frames}")
        for t in (pred, target):         # last, so that every other refusal can be had without a device
            ops._require_gpu(t, "TrialScorer.add")
        self._pending.append((group, pred, target, start, frames))

    def flush(self):
        """Builds the trial and the group table of the pending trials (sorted by group, groups in order of first appearance),
        launches ``dwn_trial_moments`` and drops the references."""
        if not self._pending:
            return
        order: dict = {}
        for i, item in enumerate(self._pending):
            key = ("g", item[0]) if item[0] is not None else ("t", i)
            order.setdefault(key, []).append(item)
        trials, groups = [], []
        for members in order.values():
            groups.append((len(trials), len(members), members[0][4]))
            trials.extend((p, y, first, frames) for _, p, y, first, frames in members)
        if self.state is None:
            self.state = torch.zeros(L.TRIAL_STATE_ROWS, self.num_neurons, dtype=torch.float64, device=trials[0][0].device)
        self.counts = ops.trial_moments(self.state, trials, groups, self.counts)
        self._flushed_groups.update(item[0] for item in self._pending if item[0] is not None)
        self._pending = []

    def compute(self) -> TrialScores:
        self.flush()
        if self.state is None:
            raise ValueError("TrialScorer.compute: no trial was added")
        scores, summary = ops.trial_scores(self.state, self.counts, self.eps, self.fev_threshold)
        return TrialScores(scores, summary, self.counts, self.fev_threshold)


@torch.no_grad()
def evaluate_trials(predictor, trials: Iterable, mouse_index: int, *, cut: FrameCut = FrameCut.submission(),
                    scorer: Optional[TrialScorer] = None, flush_every: int = 64) -> TrialScorer:
    """Runs ``predictor.predict_trial(inputs, mouse_index, to_numpy=False)`` on every ``(inputs, target[, group])`` of ``trials``
    and feeds the scorer without a copy to the host.  ``target``: ``[N, L']`` fp32 (moved to the device if it is not there; a
    numpy array is accepted), of which the first ``min(L, L')`` frames count.  Returns the scorer: ``.compute()`` gives the scores.
    A ``scorer`` shared between calls lets several fold models score their own held-out trials into one out-of-fold number, as
    the reference does (``cut`` is then the scorer's).  While no pending trial carries a group id the scorer is flushed every ``flush_every``
    trials, so the predictions of a fold need not be held at once; with groups pending everything is held until ``flush`` /
    ``compute`` (a group must be complete when it is flushed)."""
    device = predictor.model.device
    for item in trials:
        inputs, target = item[0], item[1]
        group = item[2] if len(item) > 2 else None
        pred = predictor.predict_trial(inputs, mouse_index=mouse_index, to_numpy=False)
        target = torch.as_tensor(target).to(device=device, dtype=torch.float32)
        if scorer is None:
            scorer = TrialScorer(pred.shape[0], device, cut)
        scorer.add(pred, target, group)
        if len(scorer._pending) >= flush_every and all(it[0] is None for it in scorer._pending):
            scorer.flush()
    if scorer is None:
        raise ValueError("evaluate_trials: no trials")
    return scorer


def summarise(scores: Dict[Hashable, TrialScores]) -> dict:
    """``{"correlations": {mouse: mean single-trial correlation}, "mean_correlation": their mean}``: the content of the
    reference's ``evaluate_*.json`` (src/submission.py:38-45).  One read-back per mouse."""
    correlations = {mouse: s.summary()["single_trial_corr"] for mouse, s in scores.items()}
    values = list(correlations.values())
    return {"correlations": correlations, "mean_correlation": sum(values) / len(values) if values else float("nan")}
