"""Y = A X inside a differentiable torch computation, on the library's own kernels.

    Y = spmv_amd.autograd.matmul(handle, X, values=None)

handle   an api.Handle on the current device (single GPU, not created with option "reorder")
X        (n, k) or (n,) tensor of the handle's dtype on that device; any row stride, a column stride != 1 is made contiguous first
values   None -- the matrix is a constant, only X receives a gradient -- or an nnz-element tensor of the handle's dtype: the forward pass
         makes it the handle's values (Handle.update_values; skipped when the handle already holds exactly that tensor state, told by
         the tensor's address and version counter -- a write behind the version counter, through tensor.data or a raw pointer, is not
         seen: pass a new tensor or call Handle.update_values)

forward   Handle.spmm                      Y = A X
backward  Handle.spmm_transpose(G)         dL/dX = A^T G
          Handle.sddmm(G, X)               dL/dvalues[p] = sum_c G[row(p), c] X[col(p), c]

    S = spmv_amd.autograd.sddmm(handle, U, V)          S[p] = <U[row(p)], V[col(p)]> over A's pattern, with gradients for U and V
    P = spmv_amd.autograd.row_softmax(handle, S)       softmax of S over the stored entries of every row, with a gradient for S

With matmul(handle, X, values=P) after them, softmax_rows(Q K^T on A's pattern) X -- graph attention, masked attention -- runs on the
library's kernels forward and backward (Handle.sddmm / row_softmax / spmm; Handle.row_softmax_backward, spmm, spmm_transpose, sddmm).

    O = spmv_amd.autograd.attention(handle, Q, K, V, scale=None)   the same in ONE forward pass (Handle.attention): no nnz-sized array is
                                                                   written or saved, and the handle's values are not touched
    O = spmv_amd.autograd.attention_heads(handle, Q, K, V, heads)  the same for `heads` heads side by side in the columns of Q, K and V
                                                                   (Handle.attention_heads: all heads in that one pass)

Both take a trailing keyword bias=None: a tensor of (nnz,) -- one plane, shared by all heads -- or (heads, nnz), in CSR order, added to the
scaled scores before the softmax (Handle.attention_bias), which receives a gradient (Handle.attention_bias_backward).

attention, attention_heads and attention_parts also take Q, K and V that are all torch.float16 or all torch.bfloat16 on a float32 handle
(Handle.attention_gqa_lse_16, Handle.attention_gqa_backward_16: the kernels read the 16-bit elements and compute in float32): the result and the gradients of Q, K and V have
that dtype and are the float32 results of the same function on .float() copies, each rounded once with .to(dtype); the bias and its gradient
stay float32.

Every call runs on torch's current stream.  The only module of the package that needs torch; libspmv_hip.so has no torch dependency.
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

_DTYPES = {4: torch.float32, 8: torch.float64}


def _handle_dtype(handle):
    return _DTYPES[int(handle.h.contents.data_size)]


def _handle_device(handle):
    if getattr(handle, "_ag_device", None) is None:
        handle._ag_device = int(handle.info()["device"])
    return handle._ag_device


_HALF = (torch.float16, torch.bfloat16)


def _io_dtype(handle, *tensors):
    """the dtype Q, K and V must have: the handle's, or -- on a float32 handle, when every one of them is float16 or every one bfloat16 -- that type"""
    hd = _handle_dtype(handle)
    if hd == torch.float32 and all(isinstance(t, torch.Tensor) for t in tensors) and tensors[0].dtype in _HALF and all(t.dtype == tensors[0].dtype for t in tensors):
        return tensors[0].dtype
    return hd


def _check_tensor(t, name, handle, dtype=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != (_handle_dtype(handle) if dtype is None else dtype):
        raise TypeError(f"{name} is {t.dtype}, the handle holds {_handle_dtype(handle)}")
    if t.device.type != "cuda" or t.device.index != _handle_device(handle):
        raise TypeError(f"{name} is on {t.device}, the handle lives on cuda:{_handle_device(handle)}")


def _on_current_stream(handle):
    """the handle launches on torch's current stream, asynchronously (stream-ordered like every torch op)"""
    want = (int(torch.cuda.current_stream(_handle_device(handle)).cuda_stream), True)
    if handle.attached != want:
        handle.attach_stream(want[0], async_=True)


def _token(values):
    return (values.data_ptr(), values._version)


def _apply_values(handle, values, token):
    """make `values` the handle's values unless it holds exactly that tensor state already"""
    if getattr(handle, "_values_token", None) == token:
        return
    handle.update_values(values.detach().contiguous().view(-1))
    handle._values_token = token
    handle._values_ref = values.detach()   # the address in the token stays taken while the token stands


def _block(t, k):
    """2-D operand the C side can address: column stride 1, row stride >= k"""
    if (k > 1 and t.stride(1) != 1) or t.stride(0) < k:
        return t.contiguous()
    return t


class _MatMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle, X, values):
        one_d = X.dim() == 1
        X2 = _block(X.detach().unsqueeze(1) if one_d else X.detach(), 1 if one_d else X.shape[1])
        _on_current_stream(handle)
        token = None
        if values is not None:
            token = _token(values)
            _apply_values(handle, values, token)
        Y = handle.spmm(X2)
        ctx.handle, ctx.token, ctx.one_d = handle, token, one_d
        ctx.save_for_backward(X2 if values is not None and ctx.needs_input_grad[2] else None, values)
        return Y[:, 0] if one_d else Y

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        handle = ctx.handle
        X2, values = ctx.saved_tensors
        G2 = G.unsqueeze(1) if ctx.one_d else G
        G2 = _block(G2, G2.shape[1])
        _on_current_stream(handle)
        if values is not None:   # A^T G and the pattern's gradient belong to the forward pass's matrix
            _apply_values(handle, values, ctx.token)
        dX = dV = None
        if ctx.needs_input_grad[1]:
            dX = handle.spmm_transpose(G2)
            dX = dX[:, 0] if ctx.one_d else dX
        if ctx.needs_input_grad[2]:
            dV = handle.sddmm(G2, X2).view(values.shape)
        return None, dX, dV


def matmul(handle, X, values=None):
    """A X with gradients for X and, when given, for the matrix values (see the module's docstring)."""
    if handle.multi_gpus() > 0:
        raise ValueError("multi-GPU handles (option \"gpus\") are not differentiable")
    if handle.h.contents.Level_3_opt_used:
        raise ValueError("handles created with option \"reorder\" are not differentiable: the resident matrix is P A P^T")
    _check_tensor(X, "X", handle)
    if X.dim() not in (1, 2) or X.shape[0] != handle.n:
        raise ValueError(f"X must be ({handle.n}, k) or ({handle.n},), not {tuple(X.shape)}")
    if X.dim() == 2 and X.shape[1] < 1:
        raise ValueError("X needs at least one column")
    if values is not None:
        _check_tensor(values, "values", handle)
        if values.numel() != handle.nnz:
            raise ValueError(f"values has {values.numel()} elements, the matrix {handle.nnz} non-zeros")
    return _MatMul.apply(handle, X, values)


def _check_handle(handle):
    if handle.multi_gpus() > 0:
        raise ValueError("multi-GPU handles (option \"gpus\") are not differentiable")
    if handle.h.contents.Level_3_opt_used:
        raise ValueError("handles created with option \"reorder\" are not differentiable: the resident matrix is P A P^T")


class _RowSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle, scores):
        _on_current_stream(handle)
        P = handle.row_softmax(scores.detach().contiguous().view(-1)).view(scores.shape)
        ctx.handle = handle
        ctx.save_for_backward(P)
        return P

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        (P,) = ctx.saved_tensors
        _on_current_stream(ctx.handle)
        return None, ctx.handle.row_softmax_backward(P.view(-1), G.contiguous().view(-1)).view(G.shape)


def row_softmax(handle, scores):
    """P[p] = exp(scores[p] - max) / sum over the stored entries of p's row of the handle's pattern (Handle.row_softmax), with the gradient
    dL/dscores = P * (G - sum over the row of P * G) (Handle.row_softmax_backward).  scores: an nnz-element tensor of the handle's dtype on
    its device, in CSR order.  A's values and columns play no part."""
    _check_handle(handle)
    _check_tensor(scores, "scores", handle)
    if scores.numel() != handle.nnz:
        raise ValueError(f"scores has {scores.numel()} elements, the matrix {handle.nnz} non-zeros")
    return _RowSoftmax.apply(handle, scores)


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle, U, V):
        k = U.shape[1]
        U2, V2 = _block(U.detach(), k), _block(V.detach(), k)
        _on_current_stream(handle)
        S = handle.sddmm(U2, V2)
        ctx.handle = handle
        ctx.save_for_backward(U2 if ctx.needs_input_grad[2] else None, V2 if ctx.needs_input_grad[1] else None)
        return S

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        handle = ctx.handle
        U2, V2 = ctx.saved_tensors
        dU = dV = None
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None
        if handle.nnz == 0:   # no stored entry: A_G is the zero matrix
            return None, (V2.new_zeros((handle.m, V2.shape[1])) if ctx.needs_input_grad[1] else None), \
                (U2.new_zeros((handle.n, U2.shape[1])) if ctx.needs_input_grad[2] else None)
        _on_current_stream(handle)
        # A_G = A's pattern with values G, for the duration: the handle's own values, and what matmul() remembers of them, come back below
        keep, token, ref = handle._keep[2], getattr(handle, "_values_token", None), getattr(handle, "_values_ref", None)
        Gv = G.contiguous().view(-1)
        try:
            handle.update_values(Gv)
            if ctx.needs_input_grad[1]:
                dU = handle.spmm(V2)
            if ctx.needs_input_grad[2]:
                dV = handle.spmm_transpose(U2)
        finally:
            handle.update_values(keep)
            handle._values_token, handle._values_ref = token, ref
        return None, dU, dV


def sddmm(handle, U, V):
    """S[p] = sum_c U[row(p), c] * V[col(p), c] over the handle's pattern (Handle.sddmm), with gradients for U and V: with A_G = A's pattern
    holding G = dL/dS as values, dL/dU = A_G V (Handle.spmm) and dL/dV = A_G^T U (Handle.spmm_transpose); only the gradients asked for are
    computed.  U: (m, k), V: (n, k), of the handle's dtype on its device.

    A backward pass costs two Handle.update_values: G becomes the handle's values for the two products, then the previous values are put
    back -- the array the handle held, and what matmul() remembers about it -- so a later matmul(handle, X), with values=None or with the
    earlier tensor, and Handle.spmv / spmv_transpose multiply what they did before."""
    _check_handle(handle)
    _check_tensor(U, "U", handle)
    _check_tensor(V, "V", handle)
    if U.dim() != 2 or V.dim() != 2 or U.shape[0] != handle.m or V.shape[0] != handle.n or U.shape[1] != V.shape[1] or U.shape[1] < 1:
        raise ValueError(f"U must be ({handle.m}, k) and V ({handle.n}, k) with k >= 1, not {tuple(U.shape)} and {tuple(V.shape)}")
    return _Sddmm.apply(handle, U, V)


def _bias_planes(bias):
    """the bias as the C side can address it: detached -- a reference, not a copy, unless its layout has to be mended"""
    if bias is None:
        return None
    b = bias.detach()
    return b.contiguous() if b.dim() == 1 else _block(b, b.shape[1])


def _bias_grad(dB, bias):
    """dL/dbias from the per-head planes dB (heads, nnz): a shared plane's is their sum -- torch's sum, whose order is torch's business"""
    if dB is None:
        return None
    return dB.sum(0) if bias.dim() == 1 and dB.shape[0] > 1 else dB.view(bias.shape)


def _zero_grads(Q2, K2, V2, B2, need, need_b):
    """no stored entry: O is zero whatever Q, K and V are"""
    return (torch.zeros_like(Q2) if need[0] else None), (torch.zeros_like(K2) if need[1] else None), (torch.zeros_like(V2) if need[2] else None), \
        (torch.zeros_like(B2) if need_b else None)


def _attention_backward_composed(handle, scale, Q2, K2, V2, B2, G, need, need_b):
    """-> (dQ, dK, dV, dB) of attention(): S and P computed again and the existing operations composed, only for the gradients asked for"""
    need_q, need_k, need_v = need
    dQ = dK = dV = dB = None
    if not (need_q or need_k or need_v or need_b):
        return None, None, None, None
    if handle.nnz == 0:
        return _zero_grads(Q2, K2, V2, B2, need, need_b)
    _on_current_stream(handle)
    G2 = _block(G, G.shape[1])
    S = handle.sddmm(Q2, K2)
    S.mul_(scale)
    if B2 is not None:
        S.add_(B2.view(-1))   # a rounding of its own after the scaling's: the fused kernels' two steps
    P = handle.row_softmax(S, out=S)
    # A_P, then A_dS = A's pattern with those values, for the duration: the handle's own values, and what matmul() remembers of them, come back below
    keep, token, ref = handle._keep[2], getattr(handle, "_values_token", None), getattr(handle, "_values_ref", None)
    try:
        if need_v:
            handle.update_values(P)
            dV = handle.spmm_transpose(G2)
        if need_q or need_k or need_b:
            dP = handle.sddmm(G2, V2)
            dS = handle.row_softmax_backward(P, dP, out=dP)
            if need_b:   # the bias enters after the scaling: its gradient is dS before it
                dB = dS.clone().view(B2.shape) if need_q or need_k else dS.view(B2.shape)
        if need_q or need_k:
            dS.mul_(scale)
            handle.update_values(dS)
            if need_q:
                dQ = handle.spmm(K2)
            if need_k:
                dK = handle.spmm_transpose(Q2)
    finally:
        handle.update_values(keep)
        handle._values_token, handle._values_ref = token, ref
    return dQ, dK, dV, dB


def _per_head_backward(handle, heads, kv_heads, acc, call, Q2, K2, V2, B2, G2, need, need_b):
    """-> (dQ, dK, dV, dB) from one single-head backward per query head: call(Q, K, V, B, G, dQ, dK, dV, dB) on head h's column slices -- K and V
    those of its group, h // (heads // kv_heads) -- and on its plane of the bias and of dB, written into the slices of full-width gradients.
    dK and dV of a group are its heads' terms added in torch in ascending head, in the dtype `acc` -- the first assigned, the others += -- and
    brought to Q2's dtype once at the end: the fused calls' chain and their one rounding, so both modes give the same bits."""
    gs, k, dv = heads // kv_heads, Q2.shape[1] // heads, V2.shape[1] // kv_heads
    dQ = torch.empty_like(Q2, memory_format=torch.contiguous_format) if need[0] else None
    dK = torch.empty(K2.shape, dtype=acc, device=K2.device) if need[1] else None
    dV = torch.empty(V2.shape, dtype=acc, device=V2.device) if need[2] else None
    dB = B2.new_empty((heads, handle.nnz)) if need_b else None   # of the bias' dtype: the handle's
    tK = torch.empty((handle.n, k), dtype=acc, device=K2.device) if need[1] and gs > 1 else None   # one head's term of dK / dV: what the group's later heads add
    tV = torch.empty((handle.n, dv), dtype=acc, device=V2.device) if need[2] and gs > 1 else None
    for h in range(heads):
        g, first = h // gs, h % gs == 0
        cq, co, ck, cv = slice(h * k, (h + 1) * k), slice(h * dv, (h + 1) * dv), slice(g * k, (g + 1) * k), slice(g * dv, (g + 1) * dv)
        oK = None if dK is None else (dK[:, ck] if first else tK)
        oV = None if dV is None else (dV[:, cv] if first else tV)
        call(Q2[:, cq], K2[:, ck], V2[:, cv], None if B2 is None else (B2 if B2.dim() == 1 else B2[h]), G2[:, co],
             None if dQ is None else dQ[:, cq], oK, oV, None if dB is None else dB[h])
        if not first:   # (..(first + second) + ..) + this one: plain additions in ascending head
            if dK is not None:
                dK[:, ck] += tK
            if dV is not None:
                dV[:, cv] += tV
    if acc != Q2.dtype:
        dK, dV = (None if dK is None else dK.to(Q2.dtype)), (None if dV is None else dV.to(Q2.dtype))
    return dQ, dK, dV, _bias_grad(dB, B2)


def _attention_backward(handle, heads, kv_heads, scale, mode, Q2, K2, V2, B2, G, need, need_b):
    """-> (dQ, dK, dV, dB) of attention() (heads None) and attention_heads() in the `backward=` mode asked for, only for the gradients asked for.
    "composed": the existing operations composed (_attention_backward_composed), in float32 on widened copies of 16-bit tensors, the gradients
    rounded with .to(dtype).  "fused": ONE call of the Handle method of the forward's rung.  "per_head": one single-head call per head
    (_per_head_backward) -- spmv_hip_attention_backward without a bias or kv_heads, else spmv_hip_attention_bias_backward with heads = 1; on
    16-bit tensors spmv_hip_attention_gqa_backward_16 with 1, 1, a group's terms asked for in float32.  No mode touches the handle's values but
    "composed", which puts them back; 16-bit tensors are read as they are, the bias gradient stays float32."""
    from . import api
    if not (any(need) or need_b):
        return None, None, None, None
    half = Q2.dtype in _HALF
    if mode == "composed":
        if not half:
            return _attention_backward_composed(handle, scale, Q2, K2, V2, B2, G, need, need_b)
        out = _attention_backward_composed(handle, scale, Q2.float(), K2.float(), V2.float(), B2, G.float(), need, need_b)
        return (*(None if g is None else g.to(Q2.dtype) for g in out[:3]), out[3])
    if (half or heads is not None) and handle.nnz == 0:   # attention(backward="fused") in the handle's dtype has the library write its zeros
        return _zero_grads(Q2, K2, V2, B2, need, need_b)
    _on_current_stream(handle)
    G2 = _block(G.to(Q2.dtype), G.shape[1])   # dL/dO arrives in O's dtype, which is Q's: a cast only where someone changed it
    h = 1 if heads is None else heads
    kv = h if kv_heads is None else kv_heads
    if mode == "fused":   # every head in one call
        if half:
            grads = handle.attention_gqa_backward_16(Q2, K2, V2, B2, G2, h, kv, scale, need=(*need, need_b))
        elif kv_heads is not None:
            grads = handle.attention_gqa_backward(Q2, K2, V2, B2, G2, h, kv, scale, need=(*need, need_b))
        elif B2 is not None:
            grads = handle.attention_bias_backward(Q2, K2, V2, B2, G2, h, scale, need=(*need, need_b))
        elif heads is None:
            grads = (*handle.attention_backward(Q2, K2, V2, G2, scale, need=need), None)
        else:
            grads = (*handle.attention_heads_backward(Q2, K2, V2, G2, h, scale, need=need), None)
        return (*grads[:3], _bias_grad(grads[3], B2))
    csr = (handle.h, handle.m, *handle._keep)
    if half:   # a group's sums are made in float32 and rounded once
        return _per_head_backward(handle, h, kv, Q2.dtype if h == kv else torch.float32, lambda q, k, v, b, g, dq, dk, dv, db: api.attention_gqa_backward_16(
            *csr, 1, 1, q, k, v, b, g, None, None, dq, dk, dv, db, scale), Q2, K2, V2, B2, G2, need, need_b)
    if kv_heads is None and B2 is None:
        return _per_head_backward(handle, h, kv, Q2.dtype, lambda q, k, v, b, g, dq, dk, dv, db: api.attention_backward(
            *csr, q, k, v, g, dq, dk, dv, scale), Q2, K2, V2, B2, G2, need, need_b)
    return _per_head_backward(handle, h, kv, Q2.dtype, lambda q, k, v, b, g, dq, dk, dv, db: api.attention_bias_backward(
        *csr, 1, q, k, v, b, g, dq, dk, dv, db, scale), Q2, K2, V2, B2, G2, need, need_b)


class _Attention(torch.autograd.Function):
    """attention() (heads None) and attention_heads() in every `backward=` mode, in the handle's dtype and on float16 / bfloat16 Q, K and V.
    Forward: ONE call of the narrowest rung that serves -- Handle.attention, attention_heads, attention_bias with a bias, attention_gqa with
    kv_heads; Handle.attention_gqa_lse_16 with O in their dtype (no L) for 16-bit tensors.  It saves Q, K and V -- K and V at their own, narrow,
    width -- and a reference to the bias: nothing nnz-sized but the caller's own.  Backward: _attention_backward"""

    @staticmethod
    def forward(ctx, handle, Q, K, V, heads, kv_heads, scale, mode, bias=None):
        Q2, K2, V2 = _block(Q.detach(), Q.shape[1]), _block(K.detach(), K.shape[1]), _block(V.detach(), V.shape[1])
        B2 = _bias_planes(bias)
        _on_current_stream(handle)
        h = 1 if heads is None else heads
        if Q2.dtype in _HALF:
            O, _ = handle.attention_gqa_lse_16(Q2, K2, V2, h, h if kv_heads is None else kv_heads, B2, scale, want_l=False)
        elif kv_heads is not None:
            O = handle.attention_gqa(Q2, K2, V2, heads, kv_heads, B2, scale)
        elif B2 is not None:
            O = handle.attention_bias(Q2, K2, V2, h, B2, scale)
        else:
            O = handle.attention(Q2, K2, V2, scale) if heads is None else handle.attention_heads(Q2, K2, V2, heads, scale)
        ctx.handle, ctx.heads, ctx.kv_heads, ctx.scale, ctx.mode = handle, heads, kv_heads, scale, mode
        ctx.save_for_backward(Q2, K2, V2, B2)
        return O

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        Q2, K2, V2, B2 = ctx.saved_tensors
        need = tuple(bool(x) for x in ctx.needs_input_grad[1:4])
        dQ, dK, dV, dB = _attention_backward(ctx.handle, ctx.heads, ctx.kv_heads, ctx.scale, ctx.mode, Q2, K2, V2, B2, G, need,
                                             B2 is not None and bool(ctx.needs_input_grad[8]))
        return None, dQ, dK, dV, None, None, None, None, dB


class _AttentionHeads(_Attention):
    """_Attention under the name that attention_heads() without kv_heads has in a graph: its grad_fn tells that kv_heads=None took no new path"""


def _check_bias(bias, handle, heads):
    if bias is None:
        return
    _check_tensor(bias, "bias", handle)
    if tuple(bias.shape) not in ((handle.nnz,), (heads, handle.nnz)):
        raise ValueError(f"bias must be ({handle.nnz},) or ({heads}, {handle.nnz}), not {tuple(bias.shape)}")


def attention_heads(handle, Q, K, V, heads, scale=None, backward="per_head", *, bias=None, kv_heads=None):
    """`heads` attention heads over the handle's pattern (Handle.attention_heads: one fused pass for all heads), with gradients for Q, K and
    V.  Q: (m, heads * k), K: (n, heads * k), V: (n, heads * dv) hold the heads side by side -- a (rows, heads, k) tensor reshaped to two
    dimensions --, of the handle's dtype on its device; the result is (m, heads * dv).  scale: a Python number, None means 1 / sqrt(k) with k
    one head's width; it receives no gradient.  Head h is attention() on the h-th column slices, to the bit.

    The forward pass saves Q, K and V only and neither reads nor changes the handle's values.  The backward pass calls
    spmv_hip_attention_backward once per head on column-slice views of Q, K, V and G; each call writes the matching slices of full-width
    dQ, dK and dV, only for the gradients asked for -- no Handle.update_values, the handle multiplies the same matrix throughout.  Every head
    slice of a gradient has the bits of attention(..., backward="fused") on that head's slices.

    backward="fused" routes the backward pass to ONE Handle.attention_heads_backward call (spmv_hip_attention_heads_backward) instead: two
    passes over the pattern per group of heads, the head loop inside the kernels, so the pattern, the chunking and the launches are paid per
    group and not per head.  The group is all heads when 2 * heads * nnz values fit an eighth of the device's memory (option
    "attention_backward_heads" sets another bound); the handle then holds that many values instead of 2 * nnz.  The gradients have the
    bits of the default mode.

    bias: None, or a tensor of (nnz,) -- one plane shared by all heads -- or (heads, nnz), in CSR order, added to the scaled scores before the
    softmax (Handle.attention_bias; t = (s * scale) + bias, two roundings).  It receives a gradient: dL/dbias[h, p] = P (dP - D) of head h
    (Handle.attention_bias_backward, in the same call as dQ, dK, dV; per head in the default mode, on plane h); a shared plane's gradient is the
    sum of the heads' planes -- torch's sum, whose order is not part of the contract.  A -inf entry masks that entry for that head.  The forward
    pass saves Q, K, V and a reference to the bias; a bias that needs no gradient gets none computed.

    kv_heads: None means `heads` -- everything above, untouched.  Otherwise grouped-query attention (Handle.attention_gqa): K is
    (n, kv_heads * k) and V (n, kv_heads * dv), heads a multiple of kv_heads, and query head h uses K / V head h // (heads // kv_heads) -- K and V
    are never expanded and are saved at their narrow width.  backward="fused" is one Handle.attention_gqa_backward call; the default mode calls
    the single-head backward per query head on its group's K / V slices and accumulates dK and dV of a group in torch in ascending head (the first
    head assigned, the others +=), which is the fused call's chain: both modes give the same bits.  The bias stays per QUERY head.

    16-bit tensors: on a float32 handle Q, K and V may all be torch.float16 or all torch.bfloat16 (mixed dtypes, or 16-bit tensors on a float64
    handle, are a TypeError).  The forward is then ONE Handle.attention_gqa_lse_16 call -- the kernels read the 16-bit elements, compute in float32
    and round O once -- and the backward reads them as they are too (Handle.attention_gqa_backward_16; no float32 copy of Q, K, V or dL/dO):
    backward="fused" is ONE such call with 16-bit gradients, the default mode one call per head on 16-bit column slices (a group's dK and dV added
    in float32 in ascending head and rounded once).  On a banded pattern the 16-bit backward is no faster than widening first;
    what it saves is the float32 twins of every operand.
    The contract: O is fp32_result.to(dtype) and every gradient of Q, K and V is fp32_gradient.to(dtype), where the
    float32 results are those of this same function on Q.float(), K.float(), V.float() with dL/dO.float(); the bias and its gradient stay float32,
    and the bias gradient has the float32 run's bits."""
    if backward not in ("per_head", "fused"):
        raise ValueError(f"backward must be 'per_head' or 'fused', not {backward!r}")
    _check_handle(handle)
    dtype = _io_dtype(handle, Q, K, V)
    for t, name in ((Q, "Q"), (K, "K"), (V, "V")):
        _check_tensor(t, name, handle, dtype)
    heads = int(heads)
    if kv_heads is not None:
        kv_heads = int(kv_heads)
        if heads < 1 or kv_heads < 1 or heads % kv_heads:
            raise ValueError(f"heads = {heads} is not a multiple of kv_heads = {kv_heads}")
        if Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or Q.shape[0] != handle.m or K.shape[0] != handle.n or V.shape[0] != handle.n or Q.shape[1] < 1 or V.shape[1] < 1:
            raise ValueError(f"Q must be ({handle.m}, heads * k), K ({handle.n}, kv_heads * k) and V ({handle.n}, kv_heads * dv) with k, dv >= 1, not {tuple(Q.shape)}, {tuple(K.shape)} and {tuple(V.shape)}")
        if Q.shape[1] % heads or K.shape[1] % kv_heads or V.shape[1] % kv_heads or Q.shape[1] // heads != K.shape[1] // kv_heads:
            raise ValueError(f"{Q.shape[1]} columns of Q, {K.shape[1]} of K and {V.shape[1]} of V are not {heads} query heads over {kv_heads} K / V heads of equal width")
        _check_bias(bias, handle, heads)
        scale = 1.0 / math.sqrt(Q.shape[1] // heads) if scale is None else float(scale)
        return _Attention.apply(handle, Q, K, V, heads, kv_heads, scale, backward, bias)
    if Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or Q.shape[0] != handle.m or K.shape[0] != handle.n or V.shape[0] != handle.n or \
            Q.shape[1] != K.shape[1] or Q.shape[1] < 1 or V.shape[1] < 1:
        raise ValueError(f"Q must be ({handle.m}, heads * k), K ({handle.n}, heads * k) and V ({handle.n}, heads * dv) with k, dv >= 1, not {tuple(Q.shape)}, {tuple(K.shape)} and {tuple(V.shape)}")
    if heads < 1 or Q.shape[1] % heads or V.shape[1] % heads:
        raise ValueError(f"{Q.shape[1]} columns of Q / K and {V.shape[1]} of V are not {heads} heads of equal width")
    _check_bias(bias, handle, heads)
    scale = 1.0 / math.sqrt(Q.shape[1] // heads) if scale is None else float(scale)   # Handle.attention_heads' default, to the bit
    return _AttentionHeads.apply(handle, Q, K, V, heads, None, scale, backward, bias)


def attention(handle, Q, K, V, scale=None, backward="composed", *, bias=None):
    """O = softmax_rows(scale * Q K^T on the handle's pattern) V (Handle.attention: one fused pass, the bits of
    matmul(h, V, values=row_softmax(h, sddmm(h, Q, K) * scale))), with gradients for Q, K and V.  Q: (m, k), K: (n, k), V: (n, dv), of the
    handle's dtype on its device; scale: a Python number, None means 1 / sqrt(k); it receives no gradient.

    The forward pass saves Q, K and V only -- nothing nnz-sized -- and neither reads nor changes the handle's values.  The backward pass
    computes S and P again (Handle.sddmm, Handle.row_softmax) and composes the existing operations, only for the gradients asked for:
    dP = sddmm(G, V), dS = row_softmax_backward(P, dP) * scale, dV = A_P^T G, dQ = A_dS K, dK = A_dS^T Q, where A_X is A's pattern holding
    X as values.  That costs up to three Handle.update_values per backward pass: one for P when dV is asked for, one for dS when dQ or dK is,
    and one that puts the previous values back -- the array the handle held, and what matmul() remembers about it -- so a later
    matmul(handle, X) and Handle.spmv / spmv_transpose multiply what they did before.

    backward="fused" computes the same gradients with ONE Handle.attention_backward call (spmv_hip_attention_backward: two passes over A, P
    and dS in handle-owned arrays): no Handle.update_values, the handle multiplies the same matrix throughout.  The gradients have the
    composition's bits whenever k > 1 and dv > 1 (at width 1 a contiguous tensor sends the composition's products down the spmv schedule,
    whose summation order is the method's own).

    bias: None, or a tensor of (nnz,) or (1, nnz) in CSR order, added to the scaled scores before the softmax (Handle.attention_bias with one
    head), which receives a gradient.  "composed" adds it in torch between * scale and row_softmax and takes dL/dbias from
    row_softmax_backward before * scale; "fused" takes it from the one Handle.attention_bias_backward call.  The same bits both ways for
    k, dv > 1.

    16-bit tensors: on a float32 handle Q, K and V may all be torch.float16 or all torch.bfloat16, as in attention_heads(): the forward is one
    Handle.attention_gqa_lse_16 call; backward="fused" is one Handle.attention_gqa_backward_16 call on the 16-bit tensors, "composed" the float32
    composition on widened copies; O is fp32_result.to(dtype) and
    every gradient fp32_gradient.to(dtype), the float32 results being those of this function on .float() copies -- for k, dv > 1: the 16-bit
    forward is always the fused kernel, and at width 1 the float32 results meant are those of backward="fused" (the composed float32 backward may
    take the spmv schedule there, whose order is the method's own); the bias and its gradient stay float32."""
    if backward not in ("composed", "fused"):
        raise ValueError(f"backward must be 'composed' or 'fused', not {backward!r}")
    _check_handle(handle)
    dtype = _io_dtype(handle, Q, K, V)
    for t, name in ((Q, "Q"), (K, "K"), (V, "V")):
        _check_tensor(t, name, handle, dtype)
    if Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or Q.shape[0] != handle.m or K.shape[0] != handle.n or V.shape[0] != handle.n or \
            Q.shape[1] != K.shape[1] or Q.shape[1] < 1 or V.shape[1] < 1:
        raise ValueError(f"Q must be ({handle.m}, k), K ({handle.n}, k) and V ({handle.n}, dv) with k, dv >= 1, not {tuple(Q.shape)}, {tuple(K.shape)} and {tuple(V.shape)}")
    _check_bias(bias, handle, 1)
    scale = 1.0 / math.sqrt(Q.shape[1]) if scale is None else float(scale)   # Handle.attention's default, to the bit
    return _Attention.apply(handle, Q, K, V, None, None, scale, backward, bias)


class _AttentionParts(torch.autograd.Function):
    """One Handle.attention_gqa_lse per part, folded left to right with Handle.attention_merge into one accumulator; the backward pass is one
    Handle.attention_gqa_backward_lse per part with the merged O and L.  The flat arguments after `scale`: Q, the parts' K, their V, their
    biases (None where a part has none)"""

    @staticmethod
    def forward(ctx, handles, heads, kv_heads, scale, Q, *rest):
        n = len(handles)
        Q2 = _block(Q.detach(), Q.shape[1])
        Ks = [_block(t.detach(), t.shape[1]) for t in rest[:n]]
        Vs = [_block(t.detach(), t.shape[1]) for t in rest[n:2 * n]]
        Bs = [_bias_planes(b) for b in rest[2 * n:3 * n]]
        half = Q2.dtype in _HALF   # 16-bit Q, K, V: every part's O and L in float32, the fold in float32, the merged O rounded once at the end
        O = L = None
        for r, h in enumerate(handles):
            _on_current_stream(h)
            if half:
                Or, Lr = h.attention_gqa_lse_16(Q2, Ks[r], Vs[r], heads, kv_heads, Bs[r], scale, out_dtype=torch.float32)
            else:
                Or, Lr = h.attention_gqa_lse(Q2, Ks[r], Vs[r], heads, kv_heads, Bs[r], scale)   # a part without entries: zeros and -inf
            if r == 0:
                O, L = Or, Lr
            else:
                handles[0].attention_merge(O, L, Or, Lr, heads, out=O, lse=L)   # the accumulator, in place
        ctx.handles, ctx.heads, ctx.kv_heads, ctx.scale = handles, heads, kv_heads, scale
        ctx.save_for_backward(Q2, *Ks, *Vs, *Bs, O, L)   # nothing nnz-sized but the caller's own biases; O and L in float32 also for 16-bit Q, K, V
        ctx.mark_non_differentiable(L)
        return (O.to(Q2.dtype) if half else O), L

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _GL):
        handles, heads, kv_heads, scale = ctx.handles, ctx.heads, ctx.kv_heads, ctx.scale
        n = len(handles)
        saved = ctx.saved_tensors
        Q2, Ks, Vs, Bs, O, L = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:1 + 3 * n], saved[-2], saved[-1]
        need = ctx.needs_input_grad[4:]
        need_q, need_k, need_v = bool(need[0]), [bool(x) for x in need[1:1 + n]], [bool(x) for x in need[1 + n:1 + 2 * n]]
        need_b = [Bs[r] is not None and bool(need[1 + 2 * n + r]) for r in range(n)]
        half = Q2.dtype if Q2.dtype in _HALF else None   # 16-bit: one Handle.attention_gqa_backward_16 per part on the tensors as they are
        G2 = _block(G if half is None else G.to(half), G.shape[1])
        live = sum(1 for r, h in enumerate(handles) if h.nnz > 0 and (need_q or need_k[r] or need_v[r] or need_b[r]))
        dq_dtype = torch.float32 if live > 1 else half   # more than one part adds to dQ: summed in float32 in part order, rounded once below
        dQ, dKs, dVs, dBs = None, [None] * n, [None] * n, [None] * n
        for r, h in enumerate(handles):
            if not (need_q or need_k[r] or need_v[r] or need_b[r]):
                continue
            if h.nnz == 0:   # no stored entry: the part contributes nothing, whatever its K and V are
                dKs[r] = torch.zeros_like(Ks[r]) if need_k[r] else None
                dVs[r] = torch.zeros_like(Vs[r]) if need_v[r] else None
                dBs[r] = torch.zeros_like(Bs[r]) if need_b[r] else None
                continue
            _on_current_stream(h)
            if half is not None:
                dq, dKs[r], dVs[r], dB = h.attention_gqa_backward_16(Q2, Ks[r], Vs[r], Bs[r], G2, heads, kv_heads, scale, O=O, L=L,
                                                                      need=(need_q, need_k[r], need_v[r], need_b[r]), dq_dtype=dq_dtype)
            else:
                dq, dKs[r], dVs[r], dB = h.attention_gqa_backward_lse(Q2, Ks[r], Vs[r], Bs[r], G2, O, L, heads, kv_heads, scale,
                                                                       need=(need_q, need_k[r], need_v[r], need_b[r]))
            dBs[r] = _bias_grad(dB, Bs[r])
            if need_q:   # the first part's, every later one added in part order
                if dQ is None:
                    dQ = dq
                else:
                    dQ += dq
        if need_q and dQ is None:
            dQ = torch.zeros_like(Q2)
        if half is not None and dQ is not None:
            dQ = dQ.to(half)   # the one rounding of a dQ summed over parts; a no-op on the 16-bit dQ of a single part
        return (None, None, None, None, dQ, *dKs, *dVs, *dBs)


def attention_parts(handles, Q, Ks, Vs, heads, scale=None, *, kv_heads=None, biases=None, return_lse=False):
    """Attention of the m query rows over a key / value set cut into PARTS, one handle per part, with gradients for Q, every K_r, V_r and bias:
    the softmax runs over the union of the parts' stored entries.  handles: a sequence of handles with the same m, dtype and device; part r is
    a handle of m x n_r with Ks[r] (n_r, kv_heads * k) and Vs[r] (n_r, kv_heads * dv) and an optional bias biases[r] ((nnz_r,) or
    (heads, nnz_r)); Q is (m, heads * k); kv_heads None means `heads`.  The result is (m, heads * dv); return_lse=True returns (O, L) with the
    merged row log-sum-exps L (heads, m), which receive no gradient.

    Forward: one Handle.attention_gqa_lse per part, folded left to right with Handle.attention_merge into one accumulator (the merge runs on
    the first handle; its matrix is not read).  It saves Q, the K_r / V_r, the merged O and L and references to the biases.  Backward: one
    Handle.attention_gqa_backward_lse per part with the merged O and L: dQ is the first part's, with every later part's added with += in part
    order; dK_r, dV_r and dB_r are each part's own (a shared bias plane's gradient is the sum of the heads' planes).  With one handle this is
    the log-sum-exp-driven backward of ordinary attention: the forward's O has Handle.attention_gqa's bits.  A part without stored entries
    contributes nothing.  No handle's values are read or changed.

    16-bit tensors: on float32 handles Q and every K_r and V_r may all be torch.float16 or all torch.bfloat16.  Each part is then one
    Handle.attention_gqa_lse_16 call with float32 O and L; the fold through Handle.attention_merge stays float32 and the merged O is rounded once at
    the end (the float32 merged O and L are what is saved).  The backward is one Handle.attention_gqa_backward_16 call per part on the 16-bit
    tensors with the saved float32 O and L: dK_r and dV_r come back in the 16-bit type; with more than one part dQ is float32 per part, summed in
    part order and rounded once, with one part it is 16-bit.  O is
    fp32_result.to(dtype) and every gradient of Q, K_r and V_r fp32_gradient.to(dtype), the float32 results being those of this function on .float()
    copies; L, the biases and their gradients stay float32."""
    handles = list(handles)
    Ks, Vs = list(Ks), list(Vs)
    biases = [None] * len(handles) if biases is None else list(biases)
    if not handles or not (len(handles) == len(Ks) == len(Vs) == len(biases)):
        raise ValueError(f"need one K, one V and (with biases) one bias or None per handle: {len(handles)} handles, {len(Ks)} K, {len(Vs)} V, {len(biases)} biases")
    heads = int(heads)
    kv_heads = heads if kv_heads is None else int(kv_heads)
    if heads < 1 or kv_heads < 1 or heads % kv_heads:
        raise ValueError(f"heads = {heads} is not a multiple of kv_heads = {kv_heads}")
    first = handles[0]
    for h in handles:
        _check_handle(h)
        if h.m != first.m or _handle_dtype(h) != _handle_dtype(first) or _handle_device(h) != _handle_device(first):
            raise ValueError("the parts' handles must have the same number of rows, dtype and device")
    dtype = _io_dtype(first, Q, *Ks, *Vs)   # the handles' dtype, or the one 16-bit type of Q and every K and V on float32 handles
    _check_tensor(Q, "Q", first, dtype)
    if Q.dim() != 2 or Q.shape[0] != first.m or Q.shape[1] < 1 or Q.shape[1] % heads:
        raise ValueError(f"Q must be ({first.m}, heads * k) with k >= 1, not {tuple(Q.shape)}")
    k = Q.shape[1] // heads
    dv = None
    for r, (h, K, V, b) in enumerate(zip(handles, Ks, Vs, biases)):
        _check_tensor(K, f"Ks[{r}]", h, dtype)
        _check_tensor(V, f"Vs[{r}]", h, dtype)
        if K.dim() != 2 or V.dim() != 2 or tuple(K.shape) != (h.n, kv_heads * k) or V.shape[0] != h.n or V.shape[1] < 1 or V.shape[1] % kv_heads:
            raise ValueError(f"part {r}: K must be ({h.n}, {kv_heads * k}) and V ({h.n}, kv_heads * dv) with dv >= 1, not {tuple(K.shape)} and {tuple(V.shape)}")
        if dv is not None and V.shape[1] // kv_heads != dv:
            raise ValueError(f"part {r}: V has heads of width {V.shape[1] // kv_heads}, the parts before it {dv}")
        dv = V.shape[1] // kv_heads
        _check_bias(b, h, heads)
    scale = 1.0 / math.sqrt(k) if scale is None else float(scale)
    O, L = _AttentionParts.apply(tuple(handles), heads, kv_heads, scale, Q, *Ks, *Vs, *biases)
    return (O, L) if return_lse else O
