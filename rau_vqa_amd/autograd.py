"""The step-level path as a torch.autograd.Function: a loss written in torch on the step's outputs.

``step(rau)`` runs ``rau.forward()`` and returns (logits [H,n,K], dopred [H,n], attprob [H,n,S]) as torch tensors
that carry a gradient function (dense clones: the row pitch of the device buffers, ``RAU.logits_pitch`` for an answer
count that is no multiple of 4, never shows, and the gradients go back dense).  ``loss.backward()`` on anything computed from them hands d loss / d output to the
step-level backward (``RAU.backward(..., out_grads=...)``, rau_backward_ext), which accumulates the PARAMETER
gradients in the ctx's flat buffers -- ``rau.zero_grads()`` before, ``rau.update()`` after, as on every other path.
The built-in terms (hop_w, select_w, att_w, merge_w) are given to ``step`` and join the same backward.

``step(rau, ..., feats=x)`` also carries the gradient to the FEATURE MAP, for a torch module in front of the library
(a CNN stage, a projection, an adapter).  x is the CUDA float tensor [n,D,S] the batch was made of::

    rau.want_feature_grad()
    x = proj(regions)                                        # any torch graph, on torch's current stream
    own = torch.cuda.ExternalStream(rau.stream())
    own.wait_stream(torch.cuda.current_stream())             # the ctx's copy of x runs behind its producer
    rau.set_batch_dev(x, tokens, lens, labels)
    logits, dopred, attprob = autograd.step(rau, hop_w, feats=x)
    (my_loss(logits) + ...).backward()                       # x.grad flows on into proj's parameters

The backward then returns a clone of ``rau.feature_grad_tensor()`` for x, ordered with events as the outputs are.

With ``rau.normalize_features()`` on, the library L2-normalises x per position itself and x.grad is the gradient at the
raw x (through the normalisation): nothing changes in the calls above.

Questions that share images: ``rau.want_feature_grad(per_image=True)``, ``rau.set_batch_dev(table, ..., image_of=idx)``
and ``step(rau, hop_w, feats=table)`` with the table [N,D,S] itself; table.grad is then the per-image sum, formed by
the library in a fixed order (the same bits from run to run, which an index_select backward does not give).

``step(rau, ..., question=q)`` does the same on the QUESTION side: q is the CUDA tensor [n,Q] (Q = 4 Rq; float32,
float16 or bfloat16) given to ``set_question``, the output of any torch question encoder -- a ``torch.nn.GRU`` over
cached text features, a ``Linear`` adapter, a language model's pooled state -- in place of the built-in LSTM::

    gru, adapt = torch.nn.GRU(300, 512).cuda(), torch.nn.Linear(512, rau.cfg.Q).cuda()
    _, h = gru(words)                                        # [1,n,512], on torch's current stream
    q = torch.tanh(adapt(h[0]))                              # [n,Q]
    own.wait_stream(torch.cuda.current_stream())             # the ctx's copy of q runs behind its producer
    rau.set_batch_dev(x, None, None, labels, question=q)     # or rau.set_question(q) on a resident batch
    logits, dopred, attprob = autograd.step(rau, hop_w, question=q)
    (my_loss(logits) + ...).backward()                       # q.grad flows on into adapt's and gru's parameters

The backward returns a clone of ``rau.question_grad_tensor()`` for q, ordered with events like the feature-map
gradient; the embed and rnn groups of the ctx receive nothing.  ``feats=`` and ``question=`` work together in one
step and one ``loss.backward()``.

``step(rau, ..., state=(c0, h0))`` opens the RECURRENCE: c0, h0 are the CUDA tensors [n,R] given to ``set_state`` -- the
state a previous question about the same images left, or the final state of an earlier segment -- and receive the
gradient at the initial state.  ``return_state=True`` adds the hop states to the outputs,
(logits, dopred, attprob, h [H,n,R], c_last [n,R]), differentiable at all five: a torch head on the per-hop state h'
(an answer-type classifier, a contrastive term) trains through the same backward, and chained segments hand the
gradient at one segment's initial state to the previous segment's final state (truncated BPTT)::

    rau.set_batch_dev(x, tokens, lens, labels, state=(c0, h0))
    logits, dopred, attprob, h, c_last = autograd.step(rau, hop_w, state=(c0, h0), return_state=True)
    (my_loss(logits) + head(h[-1]).logsumexp(1).mean()).backward()   # c0.grad, h0.grad flow on

``step(rau, ..., att_bias=b)`` opens the ATTENTION SCORE: b is the CUDA tensor [n,S] given to ``set_att_bias`` -- the
output of a small module of the caller's (box geometry -> score, a saliency head) -- and receives the gradient at the
bias, the sum of every active hop's softmax backward, in the same ``loss.backward()`` as the others::

    b = prior(geometry).float()                              # [n,S], requires grad through prior's parameters
    rau.set_batch_dev(x, tokens, lens, labels, att_bias=b)
    logits, dopred, attprob = autograd.step(rau, hop_w, att_bias=b)
    my_loss(logits).backward()                               # b.grad flows on into prior's parameters

torch is plumbing here: the forward, the backward and the update are librau's kernels; torch evaluates the
caller's loss and its gradient at the three outputs, on its own current stream.  The two streams are joined with
events only (ExternalStream + wait_stream), never with a host synchronisation.
"""
from __future__ import annotations

import torch


class _Step(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, question, c0, h0, att_bias, rau, hop_w, select_w, att_w, merge_w, return_state):
        dev = torch.device("cuda", rau.cfg.device_id)
        rau.forward()
        own = torch.cuda.ExternalStream(rau.stream(), device=dev)
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(own)                    # the outputs are ordered on the ctx's stream
        # clones: autograd owns what it hands out, the views die with the next forward
        outs = tuple(t.clone() for t in rau.output_tensors())
        if return_state:                        # h' of every hop and the last hop's c'
            cs, hs = rau.state_tensors()
            outs = outs + (hs.clone(), cs[-1].clone())
        ctx.rau, ctx.weights, ctx.dev = rau, (hop_w, select_w, att_w, merge_w), dev
        ctx.has_feats = anchor.dim() == 3       # step(feats=x): x is the recorded input, not the scalar anchor
        ctx.q_dtype = None if question is None else question.dtype   # step(question=q): q is a recorded input too
        ctx.s_dtype = None if c0 is None else c0.dtype   # step(state=(c0, h0)): so are c0 and h0
        ctx.b_dtype = None if att_bias is None else att_bias.dtype   # step(att_bias=b): and so is b
        ctx.set_materialize_grads(False)        # an unused output's gradient stays None instead of a zero tensor
        return outs

    @staticmethod
    def backward(ctx, d_logits, d_dopred, d_attprob, d_h=None, d_c_last=None):
        rau = ctx.rau
        # an output the loss did not use arrives as None and goes to the library as NULL
        grads = {k: g.contiguous().float() for k, g in
                 (("logits", d_logits), ("dopred", d_dopred), ("attprob", d_attprob)) if g is not None}
        own = torch.cuda.ExternalStream(rau.stream(), device=ctx.dev)
        own.wait_stream(torch.cuda.current_stream(ctx.dev))   # the gradients were written on torch's stream
        sgrads = {k: g.contiguous().float() for k, g in (("h", d_h), ("c_last", d_c_last)) if g is not None}
        for g in list(grads.values()) + list(sgrads.values()):
            g.record_stream(own)               # the caching allocator must not hand them out before the ctx has read them
        hop_w, select_w, att_w, merge_w = ctx.weights
        rau.backward(hop_w, select_w, att_w, merge_w, out_grads=grads, state_grads=sgrads or None)
        gx = None
        if ctx.has_feats:                       # the gradient at the feature map, for the graph in front of it
            torch.cuda.current_stream(ctx.dev).wait_stream(own)
            gx = rau.feature_grad_tensor().clone()   # [rows,D,S]: per sample, or per image of a table batch
            own.wait_stream(torch.cuda.current_stream(ctx.dev))   # the next step overwrites the buffer: behind the clone
        gq = None
        if ctx.q_dtype is not None:                  # the gradient at the attached question, for the encoder in front of it
            torch.cuda.current_stream(ctx.dev).wait_stream(own)
            gq = rau.question_grad_tensor().to(ctx.q_dtype, copy=True)   # [n,Q], in a 16-bit q's own type
            own.wait_stream(torch.cuda.current_stream(ctx.dev))   # the next step overwrites the buffer: behind the clone
        gc = gh = None
        if ctx.s_dtype is not None:                  # the gradient at the attached initial state
            torch.cuda.current_stream(ctx.dev).wait_stream(own)
            gc, gh = (t.to(ctx.s_dtype, copy=True) for t in rau.state_grad_tensors())   # [n,R] each
            own.wait_stream(torch.cuda.current_stream(ctx.dev))   # the next step overwrites the buffer: behind the clones
        gb = None
        if ctx.b_dtype is not None:                  # the gradient at the attached attention bias
            torch.cuda.current_stream(ctx.dev).wait_stream(own)
            gb = rau.att_bias_grad_tensor().to(ctx.b_dtype, copy=True).contiguous()   # [n,S], dense, in b's own type
            own.wait_stream(torch.cuda.current_stream(ctx.dev))   # the next step overwrites the buffer: behind the clone
        return (gx, gq, gc, gh, gb) + (None,) * 6   # parameter gradients live in the ctx's flat buffers


def step(rau, hop_w=None, select_w=None, att_w=None, merge_w=None, *, state=None, return_state=False,
         att_bias=None, feats=None, question=None):
    """forward of the resident batch -> (logits, dopred, attprob), differentiable at those three outputs.

    hop_w, select_w, att_w, merge_w: the built-in terms of RAU.backward, added to whatever loss the caller builds
    (hop_w None = zeros: an external-only objective, which needs no labels on the batch).  One ``backward()`` per
    ``step``; an output that does not enter the loss costs nothing.

    feats: the CUDA float tensor [n,D,S] the resident batch was made of (RAU.set_batch_dev), with the context's
    feature-map gradient on (RAU.want_feature_grad): it becomes the recorded input and receives its gradient.  For a
    resident image-table batch under want_feature_grad(per_image=True): the table [N,D,S].

    question: the CUDA tensor [n,Q] attached to the resident batch (RAU.set_question, set_batch_dev(question=)): it
    becomes a recorded input and receives the gradient at the question state.

    state: (c0, h0), the CUDA tensors [n,R] attached to the resident batch (RAU.set_state, set_batch_dev(state=)): they
    become recorded inputs and receive the gradient at the initial state of the hop chain.

    att_bias: the CUDA tensor [n,S] attached to the resident batch (RAU.set_att_bias, set_batch_dev(att_bias=)): it
    becomes a recorded input and receives the gradient at the attention bias.

    return_state: also return h [H,n,R] (h' of every hop) and c_last [n,R] (c' of the last hop), differentiable like
    the three outputs; the default stays the 3-tuple."""
    c0 = h0 = None
    if state is not None:
        c0, h0 = state
        shape = (rau.batch_size, rau.cfg.R)
        for t in (c0, h0):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == shape):
                raise ValueError(f"state must be the CUDA tensors (c0, h0), each [n,R] = {shape}, given to set_state")
        if not rau.batch_state:
            raise ValueError("step(state=...) needs the state attached: call rau.set_state(c0, h0) first")
        if not (c0.requires_grad or h0.requires_grad):   # (tensors nobody differentiates are just the attached state)
            c0 = h0 = None
    if att_bias is not None:
        if not (isinstance(att_bias, torch.Tensor) and att_bias.is_cuda and
                tuple(att_bias.shape) == (rau.batch_size, rau.cfg.S)):
            raise ValueError(f"att_bias must be the CUDA tensor [n,S] = {(rau.batch_size, rau.cfg.S)} given to "
                             f"set_att_bias")
        if not rau.batch_att_bias:
            raise ValueError("step(att_bias=...) needs the bias attached: call rau.set_att_bias(b) first")
        if not att_bias.requires_grad:   # (a tensor nobody differentiates is just the attached bias)
            att_bias = None
    x = None   # the recorded feature-map input, where there is one
    if question is not None:
        if not (isinstance(question, torch.Tensor) and question.is_cuda and
                tuple(question.shape) == (rau.batch_size, rau.cfg.Q)):
            raise ValueError(f"question must be the CUDA tensor [n,Q] = {(rau.batch_size, rau.cfg.Q)} given to "
                             f"set_question")
        if not rau.batch_question:
            raise ValueError("step(question=...) needs the question attached: call rau.set_question(q) first")
        if not question.requires_grad:   # (a tensor nobody differentiates is just the attached question)
            question = None
    if feats is not None:
        c = rau.cfg
        if not (isinstance(feats, torch.Tensor) and feats.is_cuda and feats.dim() == 3):
            raise ValueError("feats must be the CUDA tensor given to set_batch_dev")
        per_image = tuple(feats.shape) != (rau.batch_size, c.D, c.S)   # then: the table [N,D,S] of a resident table batch
        if per_image and not (tuple(feats.shape[1:]) == (c.D, c.S) and 1 <= feats.shape[0] <= rau.batch_size):
            raise ValueError(f"feats must be the CUDA tensor [n,D,S] = {(rau.batch_size, c.D, c.S)} given to "
                             f"set_batch_dev, or the image table [N,D,S] given to it with image_of")
        if not rau.feature_grad_wanted:
            raise ValueError("step(feats=...) needs the feature-map gradient: call rau.want_feature_grad() first")
        if per_image and rau.feature_grad_mode != 2:
            raise ValueError("step(feats=table) needs the per-image gradient: rau.want_feature_grad(per_image=True)")
        if feats.requires_grad:   # (a tensor nobody differentiates is a plain batch: the anchor below)
            x = feats
    if x is None:
        # a leaf that requires grad makes autograd record the node: the real leaves are the ctx's parameters
        x = torch.zeros((), device=torch.device("cuda", rau.cfg.device_id), requires_grad=True)
    return _Step.apply(x, question, c0, h0, att_bias, rau, hop_w, select_w, att_w, merge_w, bool(return_state))
