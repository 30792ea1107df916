"""The worker's parameter-arithmetic tasks. `aggregate` is the drop-in for
dasklearn/functions.py:89-106; `gradient_update` (functions.py:85-86), `chunk`
and `reconstruct_from_chunks` (functions.py:136-146) follow below.

`dasklearn/worker.py:27-31` resolves task functions with
`globals()[func_name]` over `from dasklearn.functions import *`; exporting an
`aggregate(settings, params)` with the same contract here is what lets the
worker run the HIP path unchanged (INTEGRATION.md shows the one-line hook).

params: {"models": [nn.Module], "round": int, "peer": int | None,
         optional "weights": [float]}  ->  [nn.Module]   (a list of one, as the
broker requires list/tuple results, broker.py:282-283).
"""
import logging
import threading
import time
from typing import Dict, List

from torch import nn

from dasklearn_amd.model_manager import ModelManager

logger = logging.getLogger(__name__)

__all__ = ["aggregate", "gradient_update", "chunk", "reconstruct_from_chunks", "sparsify", "aggregate_sparse",
           "quantize", "aggregate_quantized", "reset_sharers"]

# One sharer per (session, peer, kind), kept in the worker between tasks: the
# last-shared copy is the state of top-k sharing (sparsify below, kind "topk"),
# the residual and the call count that of quantised sharing (quantize, kind
# "quant", or "mx" when the task names an MX format). Guarded by a lock (a
# worker may run tasks on several threads); reset_sharers() drops every kind.
_sharers: Dict = {}
_sharers_lock = threading.Lock()


def reset_sharers(session=None) -> None:
    """Forget the sharers' state (last-shared copies, residuals, call counts)
    of `session` (params["session"] of the sparsify and quantize tasks; None:
    of every session). A process that runs one simulation after another under
    the same session key calls this between them, or the next run would start
    from the previous run's state."""
    with _sharers_lock:
        for key in [k for k in _sharers if session is None or k[0] == session]:
            del _sharers[key]


def _shared(settings, params: Dict, kind: str, want, make):
    """params["model"] (the first round's (model, 0) unwrapped) and the entry
    (want, sharer, lock) of the peer's sharer of `kind`, made by make() when
    the peer has none yet or its configuration `want` changed."""
    model = params["model"]
    if isinstance(model, tuple):  # the first round's (model, 0), functions.py:31-32
        model = model[0]
    session = params["session"] if "session" in params else getattr(settings, "session_id", None)
    key = (session, params["peer"], kind)
    want = want(model)
    with _sharers_lock:
        entry = _sharers.get(key)
        if entry is None or entry[0] != want:
            entry = _sharers[key] = (want, make(model, want), threading.Lock())
    return model, entry

# The reference builds the model to reconstruct into from its model zoo
# (functions.py:144, dasklearn.models.create_model). Out of scope here, so it
# is looked up lazily when the package runs inside the reference, and can be
# replaced (tests do) by assigning `model_factory`.
model_factory = None


def _create_model(settings):
    global model_factory
    if model_factory is None:
        try:
            from dasklearn.models import create_model  # the reference's model zoo
        except ImportError as exc:  # pragma: no cover - outside the reference
            raise ImportError("reconstruct_from_chunks needs dasklearn.models.create_model "
                              "or dasklearn_amd.functions.model_factory") from exc
        model_factory = create_model
    return model_factory(settings.dataset, architecture=settings.model)


def aggregate(settings, params: Dict) -> List[nn.Module]:
    models = params["models"]
    round_nr = params["round"]
    peer_id = params["peer"]
    weights = params["weights"] if "weights" in params else None
    if peer_id is not None:
        logger.debug("Peer %d aggregating %d models in round %d...", peer_id, len(models), round_nr)
    else:
        logger.debug("Aggregating %d models in round %d...", len(models), round_nr)

    model_manager = ModelManager(None, settings, 0)
    for idx, model in enumerate(models):
        model_manager.process_incoming_trained_model(idx, model)

    start_time = time.time()
    agg_model = model_manager.aggregate_trained_models(weights)
    logger.debug("Model aggregation took %f s.", time.time() - start_time)
    return [agg_model]


def gradient_update(settings, params: Dict) -> List[nn.Module]:
    """functions.py:85-86 -> ModelTrainer.gradient_update (model_trainer.py:133-143):
    the first step of a fresh SGD(settings.learning.{learning_rate, momentum,
    weight_decay}) on params["model"] with params["gradient_model"].gradient,
    on the GPU; needs no dataset. The input model is only read (the reference
    updates it in place): the returned model alone carries the update."""
    from dasklearn_amd.sgd import sgd_step_module
    model = params["model"]
    if isinstance(model, tuple):  # the first round's (model, 0), functions.py:31-32
        model = model[0]
    learning = settings.learning
    return [sgd_step_module(model, params["gradient_model"].gradient, learning.learning_rate, learning.momentum,
                            learning.weight_decay)]


def sparsify(settings, params: Dict) -> List:
    """New (the reference shares dense models only): params {"model", "peer",
    "k" | "ratio", optional "session"} -> [SparseModel], the k coordinates of
    the peer's model that moved most since it last shared them
    (dasklearn_amd/sparse.py). The worker keeps one TopKSharer per (session,
    peer): "session" (default: settings.session_id if it has one, else None)
    keeps simulations that share a worker process apart, and reset_sharers()
    drops the copies between runs. A peer whose k, ratio or parameter list
    changes starts over from a zero last-shared copy. A peer's sharer is
    locked while it shares, so tasks of one peer on several threads run one
    after the other."""
    from dasklearn_amd.arena import layout_of
    from dasklearn_amd.sparse import TopKSharer
    model, entry = _shared(settings, params, "topk",
                           lambda m: (params.get("k"), params.get("ratio"), layout_of(m)._signature),
                           lambda m, want: TopKSharer(m, k=want[0], ratio=want[1]))
    with entry[2]:
        return [entry[1].share(model)]


def quantize(settings, params: Dict) -> List:
    """New: params {"model", "peer", optional "bits" (8), "rounding"
    ("nearest"), "error_feedback" (False), "seed" (0), "session"} ->
    [QuantModel], the peer's model as 8- or 4-bit codes with one scale per 256
    elements (dasklearn_amd/quant.py). The worker keeps one QuantSharer per
    (session, peer), as sparsify keeps its TopKSharer and under the same lock:
    it holds the error-feedback residual and the count of shares that seeds
    the stochastic rounding. A peer whose bits, rounding, error_feedback, seed
    or parameter list changes starts over; reset_sharers() drops the state
    between runs. With params["format"] ("fp8_e4m3", "fp8_e5m2" or "fp4") the
    result is an [MXModel] instead (dasklearn_amd/mx.py: MX codes, one scale
    byte per 32 elements, nearest rounding; "bits", "rounding" and "seed" are
    not read), from an MXSharer kept the same way."""
    from dasklearn_amd.arena import layout_of
    from dasklearn_amd.quant import QuantSharer
    if "format" in params:
        from dasklearn_amd.mx import MXSharer
        model, entry = _shared(settings, params, "mx",
                               lambda m: (params["format"], bool(params.get("error_feedback", False)),
                                          layout_of(m)._signature),
                               lambda m, want: MXSharer(m, fmt=want[0], error_feedback=want[1]))
        with entry[2]:
            return [entry[1].share(model)]
    model, entry = _shared(settings, params, "quant",
                           lambda m: (params.get("bits", 8), params.get("rounding", "nearest"),
                                      bool(params.get("error_feedback", False)), params.get("seed", 0),
                                      layout_of(m)._signature),
                           lambda m, want: QuantSharer(m, bits=want[0], rounding=want[1], error_feedback=want[2],
                                                       seed=want[3]))
    with entry[2]:
        return [entry[1].share(model)]


def aggregate_quantized(settings, params: Dict) -> List[nn.Module]:
    """New: params {"model", "quant_models", optional "weights"} ->
    [nn.Module], the peer's own model averaged with its neighbours' quantised
    models, decoded on the fly; weights as `aggregate`'s, the own model's
    first. The neighbours are all QuantModels or all MXModels (ValueError for
    a list that mixes them: the two wire formats have a fused reduce each)."""
    from dasklearn_amd import mx, quant
    model = params["model"]
    if isinstance(model, tuple):
        model = model[0]
    kinds = {isinstance(qm, mx.MXModel) for qm in params["quant_models"]}
    if len(kinds) > 1:
        raise ValueError("aggregate_quantized takes integer-quantised or MX models, not a list that mixes them")
    mix = mx.mix if kinds == {True} else quant.mix
    return [mix(model, params["quant_models"], params["weights"] if "weights" in params else None)]


def aggregate_sparse(settings, params: Dict) -> List[nn.Module]:
    """New: params {"model", "sparse_models", optional "weights"} -> [nn.Module],
    the peer's own model averaged with its neighbours' sparse models, each
    counting as the peer's own value where it stayed silent; weights as
    `aggregate`'s, the own model's first."""
    from dasklearn_amd.sparse import mix
    model = params["model"]
    if isinstance(model, tuple):
        model = model[0]
    return [mix(model, params["sparse_models"], params["weights"] if "weights" in params else None)]


def chunk(settings, params: Dict) -> List:
    """functions.py:136-140: split a model's flat state_dict into n chunks."""
    from dasklearn_amd.chunk_manager import ChunkManager
    return ChunkManager.chunk_model(params["model"], params["n"])


def reconstruct_from_chunks(settings, params: Dict) -> List[nn.Module]:
    """functions.py:142-146: average every chunk index over its contributors
    (on the GPU) and load the result into a fresh model."""
    from dasklearn_amd.chunk_manager import ChunkManager
    model = _create_model(settings)
    model = ChunkManager.reconstruct_model(params["chunks"], model)
    return [model]
