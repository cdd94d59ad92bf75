"""Population structure on the device: signal and noise correlation matrices, and how well a model reproduces them.

Every score of ``evaluation.py`` is a per-neuron quantity.  This module answers the second-order questions: are two neurons
that are tuned alike in the data tuned alike in the model (``signal``: the correlation of the repeat averages), how much of the
trial-to-trial co-fluctuation does the model explain (``noise``: the correlation of the residuals about the repeat average; a
model that is deterministic given the stimulus has none beyond what behaviour and gaze give it), and which neurons have a
correlation fingerprint the model gets wrong (``compare``).  The frame cut and the "same video" groups are those of
``TrialScorer``; the responses stay on the device, ``dwn_pair_stage`` centres them chunk by chunk into a float64 operand and
``dwn_pair_syrk`` adds its product to the ``N x N`` co-moment state on the float64 matrix cores.
"""
from __future__ import annotations

from typing import Dict, Hashable, Iterable, Optional, Sequence

import torch

from . import ops
from .evaluation import FrameCut

KINDS = ("total", "signal", "noise")
SUMMARY_NAMES = ("pairs", "corr", "mean_a", "mean_b", "std_a", "std_b", "mean_abs_diff", "rms_diff")


class CorrelationMatrices:
    """``.total`` / ``.signal`` / ``.noise``: ``[N, N]`` device tensors (``None`` for a kind that was not asked for), ``.counts``
    the samples behind each (a kind without a sample is NaN everywhere) and ``.comoments(kind)`` the raw state.  Nothing here
    has been read back."""

    def __init__(self, matrices: Dict[str, torch.Tensor], states: Dict[str, torch.Tensor], counts: Dict[str, int]):
        self._states, self.counts = states, dict(counts)
        for kind in KINDS:
            setattr(self, kind, matrices.get(kind))

    def comoments(self, kind: str) -> torch.Tensor:
        """The ``[N, N]`` float64 centred co-moments ``sum (x_i - mean_i)(x_j - mean_j)`` of ``kind`` (a view of the state)."""
        return self._states[kind][:-1]

    def mean(self, kind: str) -> torch.Tensor:
        return self._states[kind][-1]

    def modes(self, kind: str, of: str = "correlation", **kw) -> "PopulationModes":
        """The leading modes (``modes``) of the correlation matrix of ``kind`` or, ``of="covariance"``, of its co-moments scaled
        by ``1 / counts[kind]``.  Keywords as ``modes`` (``k`` is required)."""
        if kind not in KINDS or kind not in self._states:
            raise ValueError(f"CorrelationMatrices.modes: kind must be one of {tuple(self._states)}, got {kind!r}")
        if of == "correlation":
            return modes(getattr(self, kind), **kw)
        if of != "covariance":
            raise ValueError(f"CorrelationMatrices.modes: of must be 'correlation' or 'covariance', got {of!r}")
        if self.counts[kind] < 1:
            raise ValueError(f"CorrelationMatrices.modes: no sample of kind {kind!r}")
        return modes(self.comoments(kind), scale=1.0 / self.counts[kind], **kw)


class PairwiseCorrelation:
    """Accumulates the responses of ONE mouse into one co-moment state per kind.  ``add`` keeps references to device tensors,
    ``flush`` merges them (one stage and one product launch per kind) and drops the references, ``compute`` flushes and
    finalises.  Group rules as ``TrialScorer``: trials with the same ``group`` id showed the same video, a group is complete when
    it is flushed, a group id seen once counts as no group.  The scorer flushes on its own once the pending columns exceed
    ``flush_frames`` — at chunk boundaries and never while a group is pending, so the state after any sequence of flushes equals
    the state after one, bit for bit."""

    def __init__(self, num_neurons: int, device, kinds: Sequence[str] = KINDS, cut: FrameCut = FrameCut(), eps: float = 1e-8,
                 flush_frames: int = 4096):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"sensorium_amd.PairwiseCorrelation: needs a GPU device (got {self.device}); the HIP path has no CPU fallback")
        self.num_neurons, self.cut, self.eps, self.flush_frames = int(num_neurons), cut, float(eps), int(flush_frames)
        if self.num_neurons < 1:
            raise ValueError("PairwiseCorrelation: num_neurons must be positive")
        self.kinds = tuple(kinds)
        if not self.kinds or any(k not in KINDS for k in self.kinds) or len(set(self.kinds)) != len(self.kinds):
            raise ValueError(f"PairwiseCorrelation: kinds must be distinct names from {KINDS}, got {tuple(kinds)}")
        if not self.eps > 0.0:
            raise ValueError("PairwiseCorrelation: eps must be positive")
        if self.flush_frames < 1:
            raise ValueError("PairwiseCorrelation: flush_frames must be positive")
        self.states: Dict[str, torch.Tensor] = {}
        self.counts: Dict[str, int] = {k: 0 for k in self.kinds}
        self._pending: list = []                 # (group key or None, responses, first, frames)
        self._flushed_groups: set = set()

    def add(self, responses: torch.Tensor, group: Optional[Hashable] = None, length: Optional[int] = None):
        """One trial: ``responses`` ``[N, L]`` fp32 device tensor (unit stride along frames, any row stride).  ``length`` trims
        the tail first (the NaN padding of a stored target)."""
        if group is not None and group in self._flushed_groups:
            raise ValueError(f"PairwiseCorrelation.add: group {group!r} was already flushed; add all trials of a group before flush()")
        t = responses
        if t.dtype != torch.float32:
            raise RuntimeError(f"sensorium_amd.PairwiseCorrelation.add: trials must be fp32 (got {t.dtype})")
        if t.dim() != 2 or t.shape[0] != self.num_neurons:
            raise ValueError(f"PairwiseCorrelation.add: a trial is [N = {self.num_neurons}, L], got {tuple(t.shape)}")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"PairwiseCorrelation.add: frames must have unit stride (got {t.stride(1)})")
        total = int(t.shape[1])
        if length is not None:
            if not 0 <= int(length) <= total:
                raise ValueError(f"PairwiseCorrelation.add: length {length} outside [0, {total}]")
            total = int(length)
        start, stop = self.cut.bounds(total)
        frames = stop - start
        if group is not None:
            for key, _, _, k in self._pending:
                if key == group and k != frames:
                    raise ValueError(f"PairwiseCorrelation.add: group {group!r} keeps {k} frames per trial, this trial keeps {frames}")
        ops._require_gpu(t, "PairwiseCorrelation.add")        # last, so that every other refusal can be had without a device
        self._pending.append((group, t, start, frames))
        if all(item[0] is None for item in self._pending) and sum(item[3] + 1 for item in self._pending) > self.flush_frames:
            self.flush()

    def flush(self):
        """Builds the tables of the pending trials (sorted by group, groups in order of first appearance) and merges them into
        every kind's state."""
        if not self._pending:
            return
        order: dict = {}
        for i, item in enumerate(self._pending):
            key = ("g", item[0]) if item[0] is not None else ("t", i)
            order.setdefault(key, []).append(item)
        # cut the table into launches of at most flush_frames columns of the widest kind, at group boundaries only
        batches, cur, cur_cols = [], [], 0
        for members in order.values():
            cols = max(ops.pair_chunk_cols(k, len(members), members[0][3]) for k in self.kinds)
            if cur and cur_cols + cols > self.flush_frames:
                batches.append(cur)
                cur, cur_cols = [], 0
            cur.append(members)
            cur_cols += cols
        batches.append(cur)
        dev = self._pending[0][1].device
        for batch in batches:
            trials, groups = [], []
            for members in batch:
                groups.append((len(trials), len(members), members[0][3]))
                trials.extend((x, first, frames) for _, x, first, frames in members)
            tables = ops.pair_tables(trials, groups, self.num_neurons, dev, "PairwiseCorrelation.flush")
            ws = None
            for kind in self.kinds:
                if kind not in self.states:
                    self.states[kind] = torch.zeros(self.num_neurons + 1, self.num_neurons, dtype=torch.float64, device=dev)
                need = sum(ops.pair_chunk_cols(kind, g[1], g[2]) for g in groups) * int(ops.L.lib.dwn_pair_ldz(self.num_neurons))
                if need and (ws is None or ws.numel() < need):
                    ws = torch.empty(need, dtype=torch.float64, device=dev)
                self.counts[kind] = ops.pair_accumulate(self.states[kind], kind, tables, self.counts[kind], ws)
        self._flushed_groups.update(item[0] for item in self._pending if item[0] is not None)
        self._pending = []

    def compute(self, dtype: torch.dtype = torch.float64) -> CorrelationMatrices:
        self.flush()
        if not self.states:
            raise ValueError("PairwiseCorrelation.compute: no trial was added")
        mats = {k: ops.pair_corr(self.states[k], self.counts[k], self.eps, dtype) for k in self.kinds}
        return CorrelationMatrices(mats, self.states, self.counts)


class PairwiseComparison:
    """How well matrix ``a`` (model) reproduces matrix ``b`` (data).  ``.per_neuron``: float64 device tensor, one Pearson
    correlation per selected neuron between its row of ``a`` and of ``b`` over the other selected neurons; ``.neurons``: the
    selection (int64 device tensor) or ``None`` for all."""

    def __init__(self, per_neuron: torch.Tensor, summary: torch.Tensor, neurons: Optional[torch.Tensor]):
        self.per_neuron, self._summary, self.neurons = per_neuron, summary, neurons

    def summary(self) -> Dict[str, float]:
        """Over all ordered pairs of selected neurons: their number, the Pearson correlation of ``a`` with ``b``, both means and
        standard deviations, the mean absolute and the RMS difference (NaN as soon as one entry is NaN): one read-back."""
        s = self._summary.cpu().tolist()
        out = dict(zip(SUMMARY_NAMES, s))
        out["pairs"] = int(s[0])
        return out

    def worst(self, k: int) -> torch.Tensor:
        """The ``k`` neurons whose fingerprint the model reproduces worst (lowest ``per_neuron``; a NaN row is not ranked) as a
        1-D int64 device tensor of neuron indices: what ``neurons=`` of ``attribution.input_gradient`` /
        ``most_exciting_input`` / ``tuning_curve`` takes as is."""
        score = torch.where(torch.isnan(self.per_neuron), torch.full_like(self.per_neuron, float("inf")), self.per_neuron)
        k = min(int(k), int(torch.isfinite(score).sum()))
        idx = torch.topk(score, k, largest=False).indices
        return idx if self.neurons is None else self.neurons[idx]


def compare(a: torch.Tensor, b: torch.Tensor, neurons=None, eps: float = 1e-8) -> PairwiseComparison:
    """Compares two ``[N, N]`` float64 device matrices (``dwn_pair_compare``); ``neurons``: an optional index sequence or
    tensor that restricts rows and columns."""
    sel = None
    if neurons is not None:
        sel = torch.as_tensor(neurons, device=a.device).flatten()
        if sel.numel() < 1:
            raise ValueError("compare: neurons is empty")
        if sel.dtype == torch.bool or sel.is_floating_point():
            raise ValueError("compare: neurons must be integer indices")
    per, summary = ops.pair_compare(a, b, None if sel is None else sel.to(torch.int32).contiguous(), eps)
    return PairwiseComparison(per, summary, None if sel is None else sel.to(torch.int64))


@torch.no_grad()
def population_structure(predictor, trials: Iterable, mouse_index: int, *, cut: FrameCut = FrameCut.submission(),
                         kinds: Sequence[str] = KINDS, flush_frames: int = 4096):
    """Runs ``predictor.predict_trial(inputs, mouse_index, to_numpy=False)`` on every ``(inputs, target[, group])`` of ``trials``
    (the iterable ``evaluate_trials`` takes), feeds one accumulator with the predictions and one with the targets, and returns
    ``(model, data, {kind: PairwiseComparison})``: two ``CorrelationMatrices`` and their comparison per kind.  ``target``:
    ``[N, L']`` fp32, of which the first ``min(L, L')`` frames count.  Nothing is copied to the host."""
    device = predictor.model.device
    model_acc = data_acc = None
    for item in trials:
        inputs, target = item[0], item[1]
        group = item[2] if len(item) > 2 else None
        pred = predictor.predict_trial(inputs, mouse_index=mouse_index, to_numpy=False)
        target = torch.as_tensor(target).to(device=device, dtype=torch.float32)
        if model_acc is None:
            model_acc = PairwiseCorrelation(pred.shape[0], device, kinds, cut, flush_frames=flush_frames)
            data_acc = PairwiseCorrelation(pred.shape[0], device, kinds, cut, flush_frames=flush_frames)
        length = min(int(pred.shape[1]), int(target.shape[1]))
        model_acc.add(pred, group, length)
        data_acc.add(target, group, length)
    if model_acc is None:
        raise ValueError("population_structure: no trials")
    model, data = model_acc.compute(), data_acc.compute()
    return model, data, {k: compare(getattr(model, k), getattr(data, k)) for k in model_acc.kinds}


MODES_SUMMARY_NAMES = ("k", "rounds", "converged", "trace", "participation_ratio", "leading_explained", "worst_relative_residual")


class PopulationModes:
    """The ``k`` leading eigenpairs of a symmetric matrix (``modes``), device tensors only: ``.values`` ``[k]`` descending,
    ``.vectors`` ``[N, k]`` with orthonormal columns (the entry of largest magnitude of a column, lowest index on ties, is
    positive; the mode of a rank the matrix does not have is an exact zero column with value 0), ``.residuals`` ``[k]`` =
    ``||A v - theta v||_2``, ``.trace`` and ``.frobenius2`` (0-d), ``.converged`` (0-d bool), ``.rounds`` (0-d int32)."""

    def __init__(self, values, vectors, residuals, moments, status):
        self.values, self.vectors, self.residuals = values, vectors, residuals
        self.trace, self.frobenius2 = moments[0], moments[1]
        self.converged, self.rounds = status[1] != 0, status[2]

    def explained(self) -> torch.Tensor:
        """``values / trace``: the share of the total variance each mode carries."""
        return self.values / self.trace

    def participation_ratio(self) -> torch.Tensor:
        """``tr(A)^2 / ||A||_F^2`` (0-d): the effective number of dimensions of the whole matrix."""
        return self.trace * self.trace / self.frobenius2

    def summary(self) -> Dict[str, float]:
        """One read-back."""
        worst = (self.residuals / self.values[0].abs()).max()
        row = torch.stack([self.rounds.to(torch.float64), self.converged.to(torch.float64), self.trace, self.participation_ratio(),
                           self.values[0] / self.trace, worst]).cpu().tolist()
        return dict(zip(MODES_SUMMARY_NAMES, [int(self.values.shape[0]), int(row[0]), bool(row[1])] + row[2:]))

    def project(self, responses: torch.Tensor, mean: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[k, L]`` float64 time courses of the modes in ``responses`` ``[N, L]`` (``mean`` ``[N]`` is subtracted first)."""
        x = responses.to(torch.float64)
        if mean is not None:
            x = x - mean.to(torch.float64)[:, None]
        return self.vectors.t() @ x


def modes(matrix: torch.Tensor, k: int, *, oversample: int = 8, max_iters: int = 64, tol: float = 1e-10, seed: int = 0,
          scale: float = 1.0) -> PopulationModes:
    """The ``k`` leading eigenpairs of the symmetric ``[N, N]`` float64 device matrix ``scale * matrix`` (any row stride ``>= N``;
    no copy is made) by block subspace iteration with Rayleigh-Ritz extraction on a block of ``min(k + oversample, N)``
    columns (``dwn_modes_solve``).  The run stops, on the device, once every residual of the first ``k`` pairs is at most ``tol *
    |values[0]|``; nothing is read back.  The intended input is positive semi-definite up to rounding (a correlation or
    covariance matrix); for an indefinite matrix the iteration finds the subspace dominant in magnitude."""
    if not isinstance(matrix, torch.Tensor) or not matrix.is_cuda:
        raise RuntimeError("sensorium_amd.population.modes: the matrix must be a GPU tensor; the HIP path has no CPU fallback")
    if matrix.dtype != torch.float64:
        raise RuntimeError(f"sensorium_amd.population.modes: the matrix must be float64 (got {matrix.dtype})")
    if matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1]:
        raise ValueError(f"population.modes: the matrix must be square, got {tuple(matrix.shape)}")
    k, oversample, N = int(k), int(oversample), int(matrix.shape[0])
    if k < 1 or k > N:
        raise ValueError(f"population.modes: k must lie in [1, N = {N}], got {k}")
    if oversample < 0 or k + oversample > ops.L.MODES_MAXP:
        raise ValueError(f"population.modes: k + oversample must lie in [k, {ops.L.MODES_MAXP}], got {k + oversample}")
    values, V, residuals, moments, status = ops.modes_solve(matrix, k, min(k + oversample, N), max_iters, tol, seed, scale)
    return PopulationModes(values[:k], V[:, :k], residuals[:k], moments, status)


class ModesComparison:
    """``.cosines`` ``[k]``: the cosines of the principal angles between two subspaces, descending; with a matrix ``B``,
    ``.captured`` = ``tr(Va^T B Va) / tr(B)`` (0-d) next to ``.own`` = ``sum(b.values) / b.trace``."""

    def __init__(self, cosines, captured, own):
        self.cosines, self.captured, self.own = cosines, captured, own

    def summary(self) -> Dict[str, float]:
        """One read-back."""
        parts = [self.cosines.max(), self.cosines.min(), self.own]
        if self.captured is not None:
            parts.append(self.captured)
        row = torch.stack(parts).cpu().tolist()
        out = {"k": int(self.cosines.shape[0]), "max_cosine": row[0], "min_cosine": row[1], "own": row[2]}
        if self.captured is not None:
            out["captured"] = row[3]
        return out


def compare_modes(a: PopulationModes, b: PopulationModes, matrix_b: Optional[torch.Tensor] = None,
                  scale_b: float = 1.0) -> ModesComparison:
    """The principal-angle cosines between the subspaces of ``a`` (model) and ``b`` (data): the singular values of ``Va^T Vb``
    (``dwn_modes_overlap``).  With ``matrix_b`` (and its ``scale_b``) also the share of the data's variance that lies in the
    model's subspace."""
    if a.vectors.shape != b.vectors.shape:
        raise ValueError(f"compare_modes: the two sets of modes differ in shape: {tuple(a.vectors.shape)} and {tuple(b.vectors.shape)}")
    cosines, moments = ops.modes_overlap(a.vectors, b.vectors, matrix_b, scale_b)
    own = b.values.sum() / b.trace
    return ModesComparison(cosines, None if moments is None else moments[2] / moments[0], own)
