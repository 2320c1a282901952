"""The classifier around the gated-GCN block: ``BertAmir55`` (``models/bert_amir5.py:544-650``)
with the block of lines 621-640 running on the HIP path.

Sub-module names, shapes and construction order follow the reference, so a reference
``state_dict`` loads unchanged (``bert.*``, ``dense``, ``lstm``, ``gc1``, ``gc2``, ``gate1``,
``gate2``, ``fc``) and ``Instructor._reset_params`` (``train.py:75-84``) initialises it the same
way.  ``forward(inputs) -> (logits, gate_reg, kl_reg, scores)`` like every live model of
``train.py:109``.  The sub-word pooling (``:600``), the gate MLPs (``:562-571``), the block (``:621-640``) and the
``scores`` / ``kl`` head (``:645-648``) run on the HIP path in inference; under autograd the gate MLPs and the
head keep the reference's PyTorch ops by default (they are trained; ``opt.ggcn_head_backward`` puts the head, and
``opt.ggcn_gate_backward`` the gate MLPs, on their HIP forward and one-launch backward), and with dropout active the gates
are dropped per
token like the reference's (``:621-625``); ``opt.ggcn_wide_backward`` reaches ``gc1`` and ``gc2`` through their constructor and
puts their backward on graphs of 33..128 nodes into one launch each where no gate dropout is active
(``dispatch.takes_wide_backward``); ``opt.ggcn_weighted_wide_backward`` reaches them the same way and does the same on a
real-valued adjacency of 33..128 nodes (``dispatch.takes_weighted_wide_backward``); ``opt.ggcn_hip_lstm`` puts the BiLSTM (``:610``) of an inference forward on the HIP
path (``recurrent.bilstm``: one projection, one recurrence launch), and ``opt.ggcn_hip_lstm_backward`` that of a training step
(``recurrent.bilstm_train``: the saving forward and a one-launch backward, float32, no autocast); ``opt.ggcn_pool_layers`` pools
BERT's layer outputs as the list they come in (``pooling.subword_pool_layers``: one launch, no ``torch.cat`` of ``:596``), and ``opt.ggcn_lstm_layers`` lets the BiLSTM's projection of an
inference forward read that list itself (``recurrent.bilstm_layers``: the pooled words ``[B,T,9216]`` are never formed).  BERT, ``dense`` and, by default,
the BiLSTM stay PyTorch-ROCm.

The two baselines of ``train.py:268-282`` are here too: ``AnchorEventDetector`` = ``BertED`` (``models/bert_ed.py:13-69``) and
``DynamicMultiPoolEventDetector`` = ``BertDM`` (``models/bertdm.py:104-201``), around ``pooling.anchor_pool_layers`` (one launch
from BERT's layer list to what their final linear reads).
"""
import os

import torch
import torch.nn as nn

from .csr import tensor_version
from . import dispatch
from .gated_block import gated_gcn_block, takes_block_path
from .gcn import GraphConvolution
from .heads import gate_mlps, scores_and_kl
from .hostops import _opted_in, _unless_opted_out, cached
from .pooling import anchor_pool_formula, anchor_pool_layers, subword_pool, subword_pool_layers
from .recurrent import LAYERS_MIN_ROWS, bilstm, bilstm_layers, bilstm_train, takes_hip_lstm, takes_hip_lstm_layers, takes_hip_lstm_train, lstm_wants_grad


class LegacyBertAdapter(nn.Module):
    """``pytorch_pretrained_bert`` call convention (``bert(ids, seg, output_all_encoded_layers=True)
    -> (list of 12 x [B,L,768], pooled)``, ``models/bert_amir5.py:591-593``: the second positional
    argument is token_type_ids, no attention mask is passed) on top of a ``transformers.BertModel``."""

    def __init__(self, hf_bert):
        super().__init__()
        self.model = hf_bert

    def forward(self, input_ids, token_type_ids=None, output_all_encoded_layers=True):
        o = self.model(input_ids=input_ids, token_type_ids=token_type_ids, output_hidden_states=True,
                       return_dict=True)
        layers = list(o.hidden_states[1:])   # the 12 encoder layers (index 0 is the embedding output)
        return (layers if output_all_encoded_layers else layers[-1]), o.pooler_output


class GatedGCNEventDetector(nn.Module):
    """``BertAmir55`` (VARIANT "55").  Subclasses mirror the other live models of ``train.py:268-282`` around the same
    block: ``GatedGCNEventDetector54`` = ``BertAmir54`` (``bert_amir5.py:434``: two-layer ``dense`` on [aspect, out,
    pooled], a Sigmoid in front of ``fc``), ``GCNEventDetectorNoGate`` = ``BertAmir55NoGate`` (``:654``: the two layers
    without gates; ``xy`` = 0.0).  Each loads its reference ``state_dict`` unchanged."""
    VARIANT = "55"

    def __init__(self, bert, opt):
        super().__init__()                                                  # bert_amir5.py:545-571 / :435-467 / :655-683
        self.device = getattr(opt, "device", None)
        self.bert = bert
        self.dropout = nn.Dropout(opt.dropout)
        self.hidden_dim = hd = 128
        self.n_layer = 12
        if self.VARIANT == "54":
            self.dense = nn.Sequential(nn.Linear(2 * 2 * hd + 768, 768), nn.Linear(768, opt.polarities_dim))   # :444-447
        else:
            self.dense = nn.Linear(2 * 2 * hd + 768 * self.n_layer, opt.polarities_dim)
        self.lstm = nn.LSTM(self.n_layer * 768, hd, bidirectional=True, batch_first=True, num_layers=1)
        self.gc1 = GraphConvolution(2 * hd, 2 * hd, opt)
        self.gc2 = GraphConvolution(2 * hd, 2 * hd, opt)
        self.gate1 = nn.Sequential(nn.Sigmoid(), nn.Linear(hd * 2, hd * 2), nn.Sigmoid(),
                                   nn.Linear(hd * 2, hd * 2), nn.Sigmoid())
        self.gate2 = nn.Sequential(nn.Sigmoid(), nn.Linear(hd * 2, hd * 2), nn.Sigmoid(),
                                   nn.Linear(hd * 2, hd * 2), nn.Sigmoid())
        if self.VARIANT == "54":
            self.fc = nn.Sequential(nn.Sigmoid(), nn.Linear(2 * 2 * hd, opt.polarities_dim))                  # :466-467
        else:
            self.fc = nn.Sequential(nn.Linear(2 * 2 * hd, opt.polarities_dim))
        # no precision asked for (opt.ggcn_precision / GGCN_PRECISION): inference picks the faster "f16mx8" whenever the
        # weights PROVE its fp16 range sufficient for this model (_proved_precision), "bf16x3" otherwise
        self._auto_precision = getattr(opt, "ggcn_precision", None) is None and "GGCN_PRECISION" not in os.environ
        self._assigned = (self.gc1.precision, self.gc2.precision)   # what _assign / the constructor last put there (_auto)
        self._proved = None
        # train.py:227 keeps the logits of an evaluation batch and nothing else; with opt.ggcn_eval_logits_only = True the
        # inference forward computes only what they need -- `out` (bert_amir5.py:640,643): the W12 tiles of the block, no
        # [B,T,H] store of x, no regulariser, no scores / kl head -- and returns (logits, None, None, None)
        self.eval_logits_only = bool(getattr(opt, "ggcn_eval_logits_only", False))
        # training: the scores / kl head (:645-648) as the differentiable ``scores_and_kl`` (one forward launch pair, one backward
        # launch + the weight product) instead of the reference's PyTorch ops.  Off by default: its sums differ from those ops'
        # in the last bits (both inside the gradient gate).
        self.head_backward = _opted_in(opt, "head_backward")
        # training: the gate MLPs (:562-571) as the differentiable ``gate_mlps`` (the saving forward launch, one backward launch
        # + the fixed-order weight products) instead of the two nn.Sequential.  Off by default, for the same reason.
        self.gate_backward = _opted_in(opt, "gate_backward")
        # inference: the BiLSTM (:610) as ``bilstm`` (one bf16x3 projection, one recurrence launch) where ``takes_hip_lstm`` holds --
        # float32 features and no gradient wanted; training and bf16 autocast keep nn.LSTM.  Off by default: the projection's
        # bf16x3 sums differ from the fp32 GEMM's in the last bits (both inside the forward gate).
        self.hip_lstm = _opted_in(opt, "hip_lstm")
        # training: the BiLSTM (:610) as the differentiable ``bilstm_train`` (the projection, the saving recurrence launch, one
        # backward launch + the fixed-order weight products) where a gradient is wanted and ``takes_hip_lstm_train`` holds;
        # bf16 autocast and the CPU keep nn.LSTM.  Independent of ``hip_lstm``; off by default, for the same reason.
        self.hip_lstm_backward = _opted_in(opt, "hip_lstm_backward")
        # the sub-word pooling (:600) straight from BERT's list of layer outputs: ``subword_pool_layers`` pools every layer into its
        # own columns in one launch instead of ``torch.cat`` (:596, a full [B,L,9216] copy) + ``subword_pool``.  Same bits, forward
        # and backward, float32 and bf16; taken where the layers are a list or tuple of GPU tensors.  Off by default.
        self.pool_layers = _opted_in(opt, "pool_layers")
        # inference: the BiLSTM's input projection straight from BERT's list of layer outputs (``bilstm_layers``: the projection's
        # loader pools the layers where they lie) and the anchor word's row from ``anchor_pool_layers``: the pooled words
        # [B,T,9216] are never formed either.  Taken where ``takes_hip_lstm_layers`` holds (float32 layers on the GPU, no gradient
        # wanted, no autocast); everything else keeps the paths above.  ``bilstm``'s bits; independent of ``hip_lstm`` and
        # ``pool_layers``.  Off by default.  Below ``lstm_layers_min_rows`` rows B*T (``opt.ggcn_lstm_layers_min_rows`` /
        # ``GGCN_LSTM_LAYERS_MIN_ROWS``; default ``recurrent.LAYERS_MIN_ROWS``, the measured break-even) the path is not taken: it
        # is slower there and only saves memory; 0 takes it at every size.
        self.lstm_layers = _opted_in(opt, "lstm_layers")
        self.lstm_layers_min_rows = int(getattr(opt, "ggcn_lstm_layers_min_rows", os.environ.get("GGCN_LSTM_LAYERS_MIN_ROWS", LAYERS_MIN_ROWS)))

    def _training_gates(self, aspect):
        """``gate1(aspect), gate2(aspect)`` of the training branches: the two nn.Sequential (under bf16 autocast they give bf16)
        or, with ``gate_backward``, the differentiable ``gate_mlps`` (float32 ``[B,H]``)."""
        if self.gate_backward:
            return gate_mlps(aspect, self.gate1, self.gate2)
        return self.gate1(aspect), self.gate2(aspect)

    F16_RANGE_MARGIN = 32752.0   # half of fp16's largest finite value
    F16MX8_WINDOW = 448.0        # include/ggcn.h GGCN_RANGE_WINDOW: beyond it an activation's fp8 correction saturates

    def _auto(self):
        """Still choosing the layers' precision ourselves?  A precision assigned to gc1 / gc2 after construction
        (``model.gc1.precision = "fp32"``) is the user's explicit choice from then on, like opt.ggcn_precision."""
        if self._auto_precision and (self.gc1.precision, self.gc2.precision) != self._assigned:
            self._auto_precision = False
        return self._auto_precision

    def _assign(self, precision):
        self.gc1.precision = self.gc2.precision = precision
        self._assigned = (precision, precision)

    def _proved_precision(self, csr, x=None):
        """"f16mx8" when every value that kernel rounds to fp16 is bounded below ``F16_RANGE_MARGIN`` by the weights alone
        AND every activation an f16mx8 main loop splits stays inside its accuracy window (``F16MX8_WINDOW``: the sticky
        range flag trips beyond it, ``range_guard`` raises) -- else "bf16x3".  The block's input is |x| < 1; where the block
        does not run as one launch (graphs of more than 32 nodes: LitBank, ACE cased) gc2's main loop splits gcn1, so its
        bound ``m1`` must stay inside the window too.  The block's input is the BiLSTM output (``:610``), |x| < 1 (o * tanh(c)); with a 0/1 adjacency a
        layer's output is a mean of hidden rows plus the bias (``gcn.py:35,41,43``), so
        ``|x.W1| <= c1 = colsum|W1|``, ``|gcn1| <= m1 = max(c1 + |b1|)``, ``|gcn1.W2| <= m1 * colsum|W2|``, and for the one-launch
        block ``|x.W12| + |mid| <= colsum|W1.W2| + |b1.W2|``.  One host read per weight update (cached on the parameters'
        version counters); weighted adjacencies and inference tensors (no version counter) keep "bf16x3"."""
        if not csr.is_binary:
            return "bf16x3"
        ps = (self.gc1.weight, self.gc1.bias, self.gc2.weight, self.gc2.bias)
        key = tuple(None if q is None else (q.data_ptr(), tensor_version(q)) for q in ps)
        if any(k is not None and k[1] is None for k in key):
            return "bf16x3"

        @torch.no_grad()
        def prove():
            w1, w2 = self.gc1.weight.detach().float(), self.gc2.weight.detach().float()
            b1 = torch.zeros_like(w1[0]) if self.gc1.bias is None else self.gc1.bias.detach().float()
            c1 = w1.abs().sum(0)
            m1 = (c1 + b1.abs()).max()
            w12 = w1 @ w2
            bound = torch.stack([m1.new_tensor(1.0), m1, m1 * w2.abs().sum(0).max(),
                                 (w12.abs().sum(0) + (b1 @ w2).abs()).max()]).max()
            return bool(torch.isfinite(bound)) and float(bound) < self.F16_RANGE_MARGIN, float(m1)
        ok, m1 = cached(self, "_proved", key, prove)   # (its own key: no device in it, and never one without a version -- above)
        if ok and not (m1 <= self.F16MX8_WINDOW):
            # gcn1 may leave the window: fine only where no main loop ever splits it -- the one-launch block, which runs only
            # without autograd (gated_gcn_block takes two launches when a gradient is wanted: gc2's main loop splits gcn1)
            before = (self.gc1.precision, self.gc2.precision)
            self.gc1.precision = self.gc2.precision = "f16mx8"
            try:
                grad = x is not None and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
                ok = x is not None and not grad and takes_block_path(x, csr, self.gc1, self.gc2)
            finally:
                self.gc1.precision, self.gc2.precision = before
        return "f16mx8" if ok else "bf16x3"

    def _takes_dropout_launches(self, x, csr):
        """Both layers draw the gates' dropout inside their own launches: gc1 on x (float32, or bfloat16 under autocast), gc2 on
        its real input, the float32 gcn1 -- on a 0/1 adjacency, or on a real-valued one where both layers have the opt-in
        ``weighted_dropout`` (``dispatch.takes_weighted_dropout``)."""
        if ((self.gc1.takes_dropout_path(x, csr) or self.gc1.takes_bf16_dropout_path(x, csr))
                and dispatch.takes_dropout(self.gc2, csr, dispatch.Input.of(x, torch.float32))):
            return True
        return (dispatch.takes_weighted_dropout(self.gc1, csr, dispatch.Input.of(x))
                and dispatch.takes_weighted_dropout(self.gc2, csr, dispatch.Input.of(x, torch.float32)))

    def forward(self, inputs):
        B = inputs["sentence_length"].shape[0]                              # :579-589
        L = int(inputs["cls_text_sep_length"].max())                        # one host sync, as :580-581
        T = int(inputs["sentence_length"].max())
        ids = inputs["cls_text_sep_indices"][:, :L]
        seg = inputs["cls_text_sep_segments_ids"][:, :L]
        transform = inputs["transform"][:, :T, :L]
        anchor = inputs["anchor_index"]
        dist = inputs["dist_to_target"][:, :T]
        adj = inputs["dependency_graph"]                                    # :589 dense slice, or a BatchedCSR
        if isinstance(adj, torch.Tensor):
            adj = adj[:, :T, :T]
        x, pooled = self.bert(ids, seg, output_all_encoded_layers=True)     # :591
        if self.lstm_layers and isinstance(x, (list, tuple)) and not torch.is_autocast_enabled("cuda"):
            tf, layers = transform.float(), x[-self.n_layer:]
        else:
            tf = layers = None
        if layers is not None and takes_hip_lstm_layers(tf, layers, self.lstm, self.lstm_layers_min_rows):
            # :596 + :600 + :604-610 in three launches: neither [B,L,9216] nor [B,T,9216] is formed (inference, float32)
            anchor_rep = self.dropout(anchor_pool_layers(tf, layers, anchor.long(), None, sides=False))
            x = bilstm_layers(tf, layers, self.lstm)
            return self._after_lstm(x, anchor_rep, pooled, anchor, adj, dist, torch.arange(B, device=x.device))
        if self.pool_layers and isinstance(x, (list, tuple)) and all(torch.is_tensor(t) and t.is_cuda for t in x[-self.n_layer:]):
            x = subword_pool_layers(transform.float(), x[-self.n_layer:])   # :596 + :600 in one launch, no [B,L,9216] copy
        else:
            x = torch.cat(x[-self.n_layer:], dim=-1)                        # :596
            x = subword_pool(transform.float(), x)                          # :600 on the HIP path (non-zeros only)
        rows = torch.arange(B, device=x.device)
        anchor_rep = self.dropout(x[rows, anchor])                          # :604-608: the anchor token's row
        if self.hip_lstm and not torch.is_autocast_enabled("cuda") and takes_hip_lstm(x, self.lstm):
            x = bilstm(x, self.lstm)                                        # :610 on the HIP path (inference, float32, no autocast)
        elif (self.hip_lstm_backward and not torch.is_autocast_enabled("cuda") and takes_hip_lstm_train(x, self.lstm)
              and lstm_wants_grad(x, self.lstm)):
            x = bilstm_train(x, self.lstm)                                  # :610 on the HIP path (training, float32, no autocast)
        else:
            x, _ = self.lstm(x)                                             # :610
        return self._after_lstm(x, anchor_rep, pooled, anchor, adj, dist, rows)

    def _after_lstm(self, x, anchor_rep, pooled, anchor, adj, dist, rows):
        """``forward`` from the BiLSTM's output on (``:615-648``)."""
        B, T = x.shape[0], x.shape[1]
        if x.dtype == torch.float16 and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
            # under bf16 autocast the ROCm LSTM still returns float16; the reference's first consumers of x (gc1's matmul,
            # gcn.py:34) cast it to bf16, so the layers are handed that bf16 tensor directly
            x = x.to(torch.bfloat16)
        aspect = x[rows, anchor]                                            # :615-618
        x = x.contiguous()
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        dropping = self.training and self.dropout.p > 0     # the reference drops whenever the module is in training mode
        v54, nogate = self.VARIANT == "54", self.VARIANT == "55nogate"
        if not grad and not dropping:
            # ---- inference: everything from `aspect` to `scores` on the HIP path, gates kept [B,H] ----
            if self._auto():
                if isinstance(adj, torch.Tensor):
                    adj = self.gc1._as_csr(adj, x)   # (the block would convert it anyway; identity-cached)
                self._assign(self._proved_precision(adj, x))
            want = ("out",) if self.eval_logits_only else None     # train.py:227: logits only -> only `out` of the block
            if nogate:   # :736-752: gc2(gc1(x)) and its max-pool -- the block with unit gates (one launch for T <= 32)
                ones = x.new_ones(B, 2 * self.hidden_dim, dtype=torch.float32)   # (float32 gates for bf16 x too)
                r = gated_gcn_block(x, adj, ones, ones, self.gc1, self.gc2, want=want)
                xy = 0.0
            else:
                gate1, gate2 = gate_mlps(aspect.contiguous(), self.gate1, self.gate2)     # :562-571,621-622, one launch
                r = gated_gcn_block(x, adj, gate1, gate2, self.gc1, self.gc2, want=want)  # :626-640, one launch (T <= 32)
                xy = r["xy"]
            if self.eval_logits_only:
                cat = [aspect, r["out"], pooled] if v54 else [anchor_rep, aspect, r["out"]]
                return self.dense(torch.cat(cat, dim=1)), None, None, None               # :533 / :643
            if v54:      # :531-536: dense on [aspect, out, pooled]; fc = Linear o Sigmoid, and sigmoid(cat) = cat(sigmoid)
                logits = self.dense(torch.cat([aspect, r["out"], pooled], dim=1))
                scores, kl = scores_and_kl(torch.sigmoid(r["x"]), torch.sigmoid(aspect), logits, self.fc[1], dist)
            else:
                logits = self.dense(torch.cat([anchor_rep, aspect, r["out"]], dim=1))     # :642-643 (dropout = identity)
                scores, kl = scores_and_kl(r["x"], aspect, logits, self.fc[0], dist)      # :645-648, one launch
            return logits, xy, kl, scores
        if self._auto():
            self._assign("bf16x3")   # training: the full-range default
        csr = adj if not isinstance(adj, torch.Tensor) else self.gc1._as_csr(adj, x)
        if nogate:
            gcn1 = self.gc1(x, csr)                                                    # :736
            xg, out, _ = self.gc2.forward_gated(gcn1, csr, want_pool_a=True)           # :748-749
            xy = 0.0
        elif dropping and self._takes_dropout_launches(x, csr):
            # ---- training with dropout on the one-launch path (graphs of <= 256 nodes; real-valued adjacency: weighted_dropout): the reference drops entries of the REPEATED [B,T,H] gates
            # (:621-625), one draw per token and feature.  The layers draw those keep factors in their own epilogues from a
            # counter-based hash of (seed, element) -- stream 1 for gate1, stream 2 for gate2 in BOTH layers, as the
            # reference's one dropped copy of gate2 serves :631 and :639 -- and again in the backward pass: nothing of
            # size [B,T,H] is materialised for the gates, and the pools stay in the layer launches. ----
            p = float(self.dropout.p)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())          # CPU generator: follows torch.manual_seed, no device sync
            # (under bf16 autocast the gate MLPs give bf16: the layers take float32 gates, the cast is differentiable)
            g1, g2 = (g.float().contiguous() for g in self._training_gates(aspect))
            gcn1, x1, y1 = self.gc1.forward_gated(x, csr, pool_gate_a=g1, pool_gate_b=g2, want_pool_a=True, want_pool_b=True,
                                                  dropout=(p, seed, (0, 1, 2)))          # :626-636
            xy = (x1 * y1).sum(1).mean()                                               # :638
            xg, out, _ = self.gc2.forward_gated(gcn1, csr, store_gate=g2, pool_gate_a=g2, want_pool_a=True,
                                                dropout=(p, seed, (2, 2, 0)))            # :639-640
            if pooled is not None and not v54:
                self.dropout(pooled)                                                   # :641 (unused; keeps the RNG stream)
        elif dropping:
            # ---- a layer off the one-launch path (weighted adjacency without ``weighted_dropout``, > 256 nodes, ...): gating, dropout and the pools as the reference's own
            # ops around the two HIP layers (three [B,T,H] temporaries) ----
            g1, g2 = self._training_gates(aspect)
            gate1 = self.dropout(g1[:, None, :].expand(-1, T, -1))                     # :621-624 (repeat, then dropout)
            gate2 = self.dropout(g2[:, None, :].expand(-1, T, -1))
            gcn1 = self.gc1(x, adj)                                                    # :626
            x1 = torch.max(gcn1 * gate1, 1)[0]                                         # :627-635
            y1 = torch.max(gcn1 * gate2, 1)[0]                                         # :631-636
            xy = (x1 * y1).sum(1).mean()                                               # :638
            xg = gate2 * self.gc2(gcn1, adj)                                           # :639
            out = torch.max(xg, dim=1)[0]                                              # :640
            if pooled is not None and not v54:
                self.dropout(pooled)                                                   # :641 (unused; keeps the RNG stream)
        else:
            gate1, gate2 = self._training_gates(aspect)                                # dropout is the identity here
            # (under bf16 autocast the gate MLPs give bf16: the block takes float32 gates, the cast is differentiable)
            r = gated_gcn_block(x, adj, gate1.float().contiguous(), gate2.float().contiguous(), self.gc1, self.gc2)   # :626-640
            xy, xg, out = r["xy"], r["x"], r["out"]
        if v54:
            pooled_d = self.dropout(pooled)                                 # :531
            out = self.dropout(out)                                         # :532
            logits = self.dense(torch.cat([aspect, out, pooled_d], dim=1))  # :533
        else:
            out = self.dropout(out)                                         # :642
            logits = self.dense(torch.cat([anchor_rep, aspect, out], dim=1))    # :643
        if self.head_backward:   # :645-648 on the HIP path, forward and backward (sigmoid(cat) = cat(sigmoid), as in inference)
            if v54:
                scores, kl = scores_and_kl(torch.sigmoid(xg), torch.sigmoid(aspect), logits, self.fc[1], dist)
            else:
                scores, kl = scores_and_kl(xg, aspect, logits, self.fc[0], dist)
            return logits, xy, kl, scores
        output_w = self.fc(torch.cat([xg, aspect[:, None, :].expand(-1, T, -1)], dim=2))   # :645
        scores = (logits[:, None, :] * output_w).sum(2)                     # :646
        kl = (torch.softmax(scores, 1) * torch.softmax(dist.float(), 1)).sum(1).mean()          # :648
        return logits, xy, kl, scores


class GatedGCNEventDetector54(GatedGCNEventDetector):
    """``BertAmir54`` (``models/bert_amir5.py:434-541``)."""
    VARIANT = "54"


class GCNEventDetectorNoGate(GatedGCNEventDetector):
    """``BertAmir55NoGate`` (``models/bert_amir5.py:654-752``)."""
    VARIANT = "55nogate"


class _AnchorBaseline(nn.Module):
    """What the two baselines of ``train.py:268-282`` share: BERT's layers -> sub-words pooled into words -> the anchor word's
    row and, for ``bertdm``, the two masked max-pools.  Where BERT returns a list or tuple of GPU tensors none of which requires
    grad (the reference freezes BERT, ``train.py:43-44``) the whole step is ONE launch, ``anchor_pool_layers``: in training as
    in inference, float32 and bf16, capturable.  Everywhere else -- a fine-tuned BERT, a tensor in place of the list,
    ``opt.ggcn_anchor_pool = False`` (or ``GGCN_ANCHOR_POOL=0``) -- it is the composed path: ``subword_pool_layers`` (a list of
    GPU tensors) or ``torch.cat`` + ``subword_pool``, then ``anchor_pool_formula``, the reference's PyTorch ops; differentiable,
    and the same bits."""
    SIDES = False

    def _setup(self, bert, opt, n_layer):
        self.device = getattr(opt, "device", None)
        self.bert = bert
        self.n_layer = n_layer
        self.dropout = nn.Dropout(opt.dropout)
        self.anchor_pool = _unless_opted_out(opt, "anchor_pool")

    def _anchor_parts(self, inputs):
        """``(anchor_rep [B,n*Dl] in BERT's dtype, pooled [B,2*n*Dl] float32)``; ``pooled`` is None for ``bert_ed``, and where the
        one launch already wrote the two side by side with no dropout to come between them (then the first is all of
        ``[B,3*n*Dl]``)."""
        L = int(inputs["cls_text_sep_length"].max())                        # one host sync, as bert_ed.py:30-31 / bertdm.py:148-149
        T = int(inputs["sentence_length"].max())
        ids = inputs["cls_text_sep_indices"][:, :L]
        seg = inputs["cls_text_sep_segments_ids"][:, :L]
        transform = inputs["transform"][:, :T, :L].float()
        anchor = inputs["anchor_index"].long()
        x, _ = self.bert(ids, seg, output_all_encoded_layers=True)          # bert_ed.py:42 / bertdm.py:161
        listed = isinstance(x, (list, tuple))
        if listed:
            x = x[-self.n_layer:]
        on_gpu = listed and all(torch.is_tensor(t) and t.is_cuda for t in x)
        length = None
        if self.SIDES:
            # (lengths kept on the host -- pinned, no sync at the two lines above -- are copied over without one)
            length = inputs["sentence_length"].long().to(anchor.device, non_blocking=True)
        if self.anchor_pool and on_gpu and not any(t.requires_grad for t in x):
            z = anchor_pool_layers(transform, x, anchor, length, sides=self.SIDES)      # one launch, no [B,T,n*Dl]
            if not self.SIDES:
                return z, None
            if not (self.training and self.dropout.p > 0):
                return z, None               # no dropout between the parts: z IS the concatenation of bertdm.py:198, bit for bit
            w = z.shape[1] // 3
            # (a bf16 value is exact in float32, and back; contiguous, so that dropout draws the mask it draws on the composed row)
            return z[:, :w].to(x[0].dtype).contiguous(), z[:, w:]
        if on_gpu:
            v = subword_pool_layers(transform, x)                           # no torch.cat of bert_ed.py:46 / bertdm.py:164
        else:
            v = subword_pool(transform, torch.cat(x, dim=-1) if listed else x)          # bert_ed.py:46,50 / bertdm.py:164,166
        if not self.SIDES:
            return anchor_pool_formula(v, anchor, sides=False), None        # bert_ed.py:55-62
        return anchor_pool_formula(v, anchor, length, sides=True)           # bertdm.py:170-194


class AnchorEventDetector(_AnchorBaseline):
    """``BertED`` (``models/bert_ed.py:13-69``, ``--model bert_ed``): the anchor word's pooled row of the 12 BERT layers,
    dropout, ``fc``.  (With bf16 layers the launch's float32 row is converted back by one small elementwise kernel.)  Loads a reference ``state_dict`` unchanged (``bert.*``, ``fc``); ``forward(inputs) -> (logits, 0, 0,
    None)``."""

    def __init__(self, bert, opt):
        super().__init__()
        self._setup(bert, opt, 12)                                          # bert_ed.py:17-21
        self.hidden_dim = getattr(opt, "hidden_dim", None)
        self.fc = nn.Linear(768 * self.n_layer, opt.polarities_dim)         # :22

    def forward(self, inputs):
        anchor_rep, _ = self._anchor_parts(inputs)
        return self.fc(self.dropout(anchor_rep)), 0, 0, None                # :65-69


class DynamicMultiPoolEventDetector(_AnchorBaseline):
    """``BertDM`` (``models/bertdm.py:104-201``, ``--model bertdm``, dynamic multi-pooling): over the last ``opt.n_layer`` BERT
    layers the anchor word's row, the max-pool over the words up to and including the anchor and the one over the words after
    it, dropout on the anchor part and on the concatenation, ``dense``.  Loads a reference ``state_dict`` unchanged (``bert.*``,
    ``dense``; the reference's ``self.m`` is a plain attribute, not a buffer); ``forward(inputs) -> (logits, 0.0, 0.0, 0.0)``."""
    SIDES = True

    def __init__(self, bert, opt):
        super().__init__()
        self._setup(bert, opt, opt.n_layer)                                 # bertdm.py:108-111
        self.dense = nn.Linear(opt.n_layer * opt.bert_dim * 3, opt.polarities_dim)      # :112

    def forward(self, inputs):
        anchor_rep, pooled = self._anchor_parts(inputs)
        x = anchor_rep if pooled is None else torch.cat((self.dropout(anchor_rep), pooled), 1)      # :197-198
        return self.dense(self.dropout(x)), 0.0, 0.0, 0.0                   # :199-201
