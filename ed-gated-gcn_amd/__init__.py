"""MI355X-native gated graph convolution: drop-in for the GCN hot path of laiviet/ed-gated-gcn.

The directory carries the reference's (hyphenated) name; import it as
``ed_gated_gcn_amd`` (the one-file alias at the repository root).

Public surface (mirrors the reference interface for this path):

* ``GraphConvolution``  -- ``models/gcn.py:9-45``: same constructor, parameters,
  ``state_dict`` and ``forward(text, adj)``.
* ``gated_gcn_block``   -- ``models/bert_amir5.py:621-640``: gate -> gc1 -> gate ->
  gc2 -> gate -> max-pool, never materialising the [B,T,H] gates.
* ``BatchedCSR``        -- many sentence graphs as one block-diagonal CSR.
* ``subword_pool``      -- ``models/bert_amir5.py:600``: ``bmm(transform, x)`` on the non-zeros only.
* ``subword_pool_layers`` -- the same on BERT's list of layer outputs, without the ``torch.cat`` of ``:596``: one launch, same bits.
* ``anchor_pool_layers`` -- the baselines' step (``models/bert_ed.py:46-62``, ``models/bertdm.py:164-198``): from that list to the
  anchor word's row and the two masked max-pools in one launch; ``anchor_pool_formula`` is its second half as PyTorch ops.
* ``AnchorEventDetector`` / ``DynamicMultiPoolEventDetector`` -- the baselines ``BertED`` and ``BertDM`` around it.
* ``bilstm``            -- ``models/bert_amir5.py:610``: the BiLSTM forward in inference, one projection and one recurrence launch.
* ``bilstm_layers``     -- ``:596,600,610`` in two launches: the projection pools BERT's layer list in its own loader (no ``[B,T,9216]``), then the recurrence.
* ``bilstm_train``      -- the same line under autograd: the saving forward and a one-launch backward (``x`` and all eight parameters).

All compute is in ``libggcn_hip.so`` (hand-written HIP for gfx950, C ABI in
``include/ggcn.h``).  There is no CPU or PyTorch fallback: without the library or
a GPU tensor every entry point raises.
"""
from ._capi import lib_path, load_library  # noqa: F401
from .csr import BatchedCSR  # noqa: F401
from .gcn import GraphConvolution  # noqa: F401
from .gated_block import gated_gcn_block  # noqa: F401
from .pooling import anchor_pool_formula, anchor_pool_layers, subword_pool, subword_pool_layers  # noqa: F401
from .heads import dense_head, gate_mlps, scores_and_kl  # noqa: F401
from .recurrent import bilstm, bilstm_layers, bilstm_train, takes_hip_lstm, takes_hip_lstm_layers, takes_hip_lstm_train  # noqa: F401
from .classifier import GatedGCNEventDetector, GatedGCNEventDetector54, GCNEventDetectorNoGate, LegacyBertAdapter  # noqa: F401
from .classifier import AnchorEventDetector, DynamicMultiPoolEventDetector  # noqa: F401

__all__ = ["GraphConvolution", "gated_gcn_block", "BatchedCSR", "subword_pool", "subword_pool_layers", "anchor_pool_layers", "anchor_pool_formula", "AnchorEventDetector", "DynamicMultiPoolEventDetector", "gate_mlps", "scores_and_kl", "bilstm", "takes_hip_lstm", "bilstm_train", "takes_hip_lstm_train", "bilstm_layers", "takes_hip_lstm_layers", "GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate", "LegacyBertAdapter",
           "load_library", "lib_path"]
