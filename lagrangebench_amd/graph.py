"""Graph primitives with autograd on the engine's current neighbor list (csrc/lb_graph.hip).

What a message-passing network written in torch needs from the graph: ``x[senders]``, ``x[receivers]`` and
``jraph.segment_sum(msg, receivers | senders, N)``.  ``Graph`` runs them as HIP kernels on the list the ``FeatureDict``
describes, in the padded layout of ``features["senders"]`` / ``["receivers"]`` ((B, E_cap), pad slots hold N):

    g = Graph(features)                      # binds features.engine and features.version
    xs = g.gather(x, "senders")              # (B, N, C) -> (B, E_cap, C); pad slots are +0.0
    agg = g.segment_sum(msg, "receivers")    # (B, E_cap, C) -> (B, N, C); pad slots are never read
    g.n_edges, g.senders, g.receivers        # (B,), (B, E_cap), (B, E_cap)

    g.degree("receivers")                    # (B, N) int32: the node's real slots
    g.segment_mean(msg, "receivers")         # segment_sum / max(degree, 1)
    g.segment_max(msg, "senders")            # (B, E_cap, C) -> (B, N, C); segment_min likewise
    a = g.segment_softmax(logits, "receivers")          # (B, E_cap, C) -> (B, E_cap, C): a softmax per node and column
    out = g.attend(logits, values, "receivers")         # (B, E_cap, H), (B, E_cap, H, D) -> (B, N, H, D), one launch
    agg = g.aggregate(msg, "receivers", ("sum", "mean", "max", "min", "std"))   # (B, E_cap, C) -> (B, N, 5, C), one launch
    g.segment_std(msg, "receivers"), g.segment_var(msg, "receivers")            # (B, E_cap, C) -> (B, N, C)

    ds = g.conv(x, w, "senders")             # (B, N, C) | (B, N, K, C), (B, E_cap, C) -> the shape of x, one launch:
                                             #   segment_sum(gather(x, "receivers") * w[..., None, :], "senders")
    e = g.pair_add(a, b)                     # (B, N, C) twice -> (B, E_cap, C): a[senders] + b[receivers]
    m = g.pair_mul(a, b)                     # ... a[senders] * b[receivers]
    dv = g.conv_vec(s, w, u, "senders")      # (B, N, C), (B, E_cap, C), (B, E_cap, K) -> (B, N, K, C): scalar -> vector channels,
                                             #   segment_sum((gather(s, "receivers") * w)[..., None, :] * u[..., :, None], "senders")
    ds = g.conv_dot(v, w, u, "senders")      # (B, N, K, C), ... -> (B, N, C): vector -> scalar, sum of w * <v[receivers], u>
    ds = g.filter_conv(x, f, weight, "senders")   # f (B, E_cap, R), weight (R, C): conv(x, f @ weight, "senders") without f @ weight

    g.reverse                                # (B, E_cap) int32: the slot of the transposed edge (r -> s) of slot (s -> r), -1 without one
    t = g.swap(msg)                          # (B, E_cap, C) -> (B, E_cap, C): msg[reverse]
    m = g.antisymmetrize(msg)                # ... msg - msg[reverse]: m_ij = -m_ji exactly; symmetrize: msg + msg[reverse]

(with un-batched features the leading B is dropped: (N, C) -> (E_cap, C)).  Trailing dimensions beyond C are folded into C
where the op is column-wise (all but ``attend``).

The sum is ordered: per node its real slots in ascending slot order, one float32 add after the other, no atomics - the
result equals a numpy float32 loop bit for bit and two calls give the same bits (torch's ``index_add_`` on the GPU uses
float atomics and does not).  The two ops are each other's adjoints - gather's backward is ``segment_sum`` over the same
role, ``segment_sum``'s backward is ``gather`` - so forward and backward are the same two kernels with the same bits.

The attention ops keep these contracts - pad slots are never read (they may hold NaN), every pad slot of an edge-shaped
result or gradient is +0.0, no float atomics, two calls give the same bits:

* ``segment_max`` starts from the node's first real slot; a further slot, in ascending slot order, replaces it only if it is
  strictly greater (ties keep the earlier slot, -0.0 then +0.0 stays -0.0; a NaN wins and stays, as ``np.maximum``).  The
  gradient goes to the winning slot alone.  ``segment_min`` mirrors it.  A node without edges gets +0.0 - jraph gives -inf /
  +inf there; like ``segment_sum`` we keep what such a node feeds onward finite.
* ``segment_mean`` is the ordered sum followed by one correctly rounded float32 division by ``max(degree, 1)``.
* ``segment_softmax`` per node and column: m = the maximum as above, e_j = expf(x_j - m), s = the ordered sum of the e_j,
  y_j = e_j / s.  Backward: y_j (d_y_j - sum_k d_y_k y_k), the sum ordered.
* ``attend(logits, values, role)`` equals ``segment_sum(segment_softmax(logits, role)[..., None] * values, role)`` bit for
  bit - the same weights, each product rounded to float32, added in ascending slot order - without the (E_cap, H, D)
  intermediate.  Its ``d_values`` has the composition's bits too; ``d_logits`` reduces over D in another order and agrees
  to rounding.

Multi-aggregator.  ``aggregate(msg, role, ops, eps)`` gives the reductions a PNA layer concatenates - any distinct names out of
``sum, mean, max, min, std, var`` - as the planes of one (B, N, A, C) result, in the order of ``ops``, from one node-parallel
launch: one walk of the row for the sum, both extrema and their winners, a second, cache-hot walk for the centred squares only
when ``std`` or ``var`` is asked for.  ``segment_std`` and ``segment_var`` are its one-plane forms.  An empty or unknown
``ops``, a name twice, or ``eps <= 0`` with ``std`` is a ``ValueError``.  Per node and column, over the real slots
j1 < ... < jd of `role` in ascending slot order (d the degree), under the contracts above:

* ``sum``: the bits of ``segment_sum``; ``mean``: ``m = fl32(sum / max(d, 1))``, the bits of ``segment_mean``; ``max`` /
  ``min``: the bits and the winning slots of ``segment_max`` / ``segment_min`` (first slot, replaced only by a strictly
  greater / smaller one, ties keep the earlier slot, a NaN wins and stays).
* ``var = fl32(q / max(d, 1))``, centred and two-pass: ``t_j = fl32(x_j - m)`` and q is the ordered float32 sum of
  ``fl32(t_j * t_j)``, the first term starting it - never ``E[x^2] - m^2``, which loses every digit once the mean is large
  against the spread.  ``std = sqrt_rn(fl32(var + eps))``, eps inside the root as PNA has it.
* A node without slots gets +0.0 in every plane, ``std`` included (not ``sqrt(eps)``).  Every step is one correctly rounded
  IEEE operation, so a numpy float32 loop reproduces every plane bit for bit.
* Backward: one edge-parallel launch writes ``d_msg`` once, +0.0 in the pad slots.  For a real slot j of node n the present
  terms are added in this fixed order, whatever the order of ``ops``, the first present one starting the sum: ``g_sum``;
  ``fl32(g_mean / d)``; ``g_max`` if j is the max winner of (n, c); ``g_min`` likewise; ``fl32(fl32(g_std * t_j) / fl32(d *
  std))``; ``fl32(fl32(fl32(2 * g_var) * t_j) / d)`` - ``t_j`` recomputed from msg and the saved mean.  A slot without a present
  term gets +0.0, so the single-op gradients of sum, mean, max and min have the bits of the separate ops'.  The forward hands
  the backward the winning slots (int32) and the float32 mean and std, allocated only when asked for; msg is saved only with
  ``std`` or ``var``.
* bfloat16: the forward and ``d_msg`` are the float32 result on the widened inputs, rounded once per stored element; the mean
  inside ``var`` and in the backward is the float32 mean, not its rounded copy (so the ``mean`` plane is rounded once, where
  ``segment_mean`` on bfloat16 rounds the sum first).

Edge messages.  ``conv``, ``pair_mul`` and ``pair_add`` are the "filter x neighbour" message of a continuous-filter or
equivariant network (SchNet's cfconv, PaiNN's ``segment_sum(Wij * x[receivers], senders)``) and the first edge Linear of a
message-passing layer, without their edge-shaped intermediates, under the same contracts:

* ``conv(x, w, role)``: ``out[i, k, c]`` is the sum over the real slots j whose `role` index is i, in ascending slot order,
  of ``fl32(x[other-role index of j, k, c] * w[j, c])`` - each product rounded to float32, the first product starts the sum,
  one float32 add per further one, +0.0 for a node without slots.  So on float32 it equals
  ``segment_sum(gather(x, other) * w[..., None, :], role)`` bit for bit.  x is (B, N, C) - trailing dimensions equal to w's
  fold into C - or (B, N, K, C) with w (B, E_cap, C) broadcast over K (a vector feature: K = 3); anything else is a
  ``ValueError``.  Backward: ``d_x = conv(d_out, w, other(role))``, the composition's bits; ``d_w[j, c]`` is the sum over k
  ascending of ``fl32(x[other index of j, k, c] * d_out[role index of j, k, c])``, +0.0 in the pad slots.  Only x and w are
  saved, and a gradient nobody asked for is not computed.
* ``pair_mul(a, b)`` = ``fl32(a[senders] * b[receivers])`` and ``pair_add(a, b)`` = ``fl32(a[senders] + b[receivers])``, a and b
  (B, N, C) -> (B, E_cap, C), +0.0 in the pad slots.  Backward: ``conv(b, d, "senders")`` and ``conv(a, d, "receivers")``;
  ``segment_sum(d, "senders")`` and ``segment_sum(d, "receivers")``.

Vector messages.  ``conv_vec`` and ``conv_dot`` couple scalar channels to vector channels through a per-edge vector ``u``
(B, E_cap, K), 1 <= K <= 9 - ``features["rel_disp"]``, or spherical harmonics up to l = 2: PaiNN's ``w_vs s_j (x) r_ij`` and
``w_sv <v_j, r_ij>``, EGNN's position update at C = 1 - without the (B, E_cap, K, C) product, under the same contracts (n(j) is
the `role` node of slot j, o(j) its other node; every product is rounded to float32, every sum starts from its first term):

* ``conv_vec(x, w, u, role)[i, k, c]``: the sum over the real slots j with n(j) = i, ascending, of
  ``fl32(fl32(x[o(j), c] * w[j, c]) * u[j, k])``; on float32 the composition written above, bit for bit.
* ``conv_dot(v, w, u, role)[i, c]``: the sum over those slots of ``fl32(w[j, c] * t[j, c])`` with ``t[j, c] = fl32(v[o(j), 0, c] *
  u[j, 0]) + fl32(v[o(j), 1, c] * u[j, 1]) + ...``, k ascending.
* They are each other's adjoints: ``d_x`` of ``conv_vec`` over `role` is ``conv_dot(d, w, u, other role)`` and ``d_v`` of
  ``conv_dot`` is ``conv_vec(d, w, u, other role)`` - the same kernels, the same bits.
* The gradients to w and u of either op come from one edge-parallel launch over a scalar-side node tensor S and a vector-side
  one V (``conv_vec``: S = x at o(j), V = d at n(j); ``conv_dot``: S = d at n(j), V = v at o(j)): ``d_w[j, c] = fl32(S[c] *
  t[j, c])`` with t formed from V and u as above, and ``d_u[j, k]`` = the sum over c of ``fl32(fl32(S[c] * w[j, c]) * V[k, c])``
  in a fixed order - the columns in consecutive blocks of 16 (the last may be short), c ascending inside a block, the block sums
  added in ascending block order - which a numpy loop reproduces.  Pad slots of both are +0.0; a gradient nobody asked for is
  neither computed nor allocated; only x / v, w and u are saved.  The gradient to u flows on to the window through
  ``differentiable_features``.
* On bfloat16 every output, ``d_u`` included, is the float32 result on the widened inputs rounded once - not the composition
  of the bfloat16 ops.

Continuous filter.  ``filter_conv(x, f, weight, role)`` is ``conv`` with the dense layer that makes its filter inside: f
(B, E_cap, R), 1 <= R <= 32, is any per-edge basis the module computed (Gaussians of ``rel_dist`` times a cutoff; its pad slots
may hold NaN), weight (R, C) is shared by the batch - the first graph op that takes a parameter.  Under the same contracts:

* The filter ``wf[j, c] = fl32(f[j, 0] * weight[0, c]) + fl32(f[j, 1] * weight[1, c]) + ...``, r ascending, the first product
  starts the sum - formed in registers, never stored; NOT torch's ``f @ weight``, whose order is unstated.  ``out[i, k, c]`` is
  ``conv``'s sum of ``fl32(x[o(j), k, c] * wf[j, c])`` over the real slots of node i in ascending slot order, +0.0 for a node
  without slots: on float32 bit for bit ``conv(x, wf, role)``.  The forward allocates its output only.
* No bias argument: a bias is a column of f - ones, or the cutoff envelope, since ``(Linear(rbf) + b) * fcut = [rbf * fcut,
  fcut] @ [W; b]``.
* Backward, from x, f and weight alone; a gradient nobody asked for is neither computed nor allocated.  With ``g[j, c] =
  fl32(x[o(j), 0, c] * d[n(j), 0, c]) + ...``, k ascending (``conv``'s ``d_w``, never stored): ``d_x = filter_conv(d, f, weight,
  other role)``, the composition's bits; ``d_f[j, r]`` = the sum over c of ``fl32(weight[r, c] * g[j, c])`` in the blocked column
  order of ``d_u`` above, +0.0 in the pad slots - it flows on to the window through ``differentiable_features``;
  ``d_weight[r, c]`` = the sum over every real slot of every trajectory of ``fl32(f[j, r] * g[j, c])`` in a two-level order: the
  flat padded slots ``b * E_cap + j`` in consecutive chunks of ``LB_GRAPH_FILTER_CHUNK`` (include/lbhip.h), per chunk a partial
  that starts at +0.0 and takes its real slots' terms in ascending order, the total from +0.0 over the partials in ascending
  chunk order.  No atomics, two calls the same bits, a numpy loop reproduces it.  One launch for ``d_x``, one for ``d_f``, two for
  ``d_weight``; the float32 partials (chunks, R, C) are the only scratch.
* bfloat16: every output, ``d_f`` and ``d_weight`` included, is the float32 result on the widened inputs rounded once; wf and g
  stay float32, so it is not the composition of the bfloat16 ops but the more accurate of the two.  A float32 weight beside
  bfloat16 x and f - a Parameter under ``TorchModel(autocast=torch.bfloat16)`` - is cast with a differentiable
  ``.to(bfloat16)``, as torch casts a Linear's weight; its gradient arrives in float32.  Every other dtype mix is a ``TypeError``.

Edge pairs.  Every op above sees an edge (s -> r) alone; ``reverse``, ``swap``, ``symmetrize`` and ``antisymmetrize`` relate it to
its transpose (r -> s) - pairwise forces with ``F_ij = -F_ji`` (linear momentum conserved by construction), symmetric edge
features, edge states that read the opposite edge's - under the same contracts (pad slots never read, +0.0 in every pad slot of a
result or gradient, no atomics, two calls the same bits):

* ``reverse`` is (B, E_cap) int32: for the real slot j of (receiver r, sender s) the slot, within its trajectory, of the edge
  (receiver s, sender r); a self-edge maps to itself; -1 where the list holds no such edge, and -1 in every pad slot.  The
  displacement is antisymmetric only up to one rounding, so a pair at the cutoff can be an edge in one direction only: the
  map says which, and ``reverse[reverse[j]] == j`` wherever ``reverse[j] >= 0``.  The engine builds it in one launch at its first
  use after a list build - each slot bisects the sorted CSR row of its sender for its receiver - and keeps it; the property is
  a copy, cached per features version.  Nothing is read back, and the sender view is not involved.
* ``swap(msg)[j] = msg[reverse[j]]``, a bit copy; ``symmetrize(msg)[j] = fl32(msg[j] + msg[reverse[j]])``;
  ``antisymmetrize(msg)[j] = fl32(msg[j] - msg[reverse[j]])`` - one float32 operation, no rounding for ``swap``.  msg is
  (B, E_cap, C); trailing dimensions fold into C.
* The unpaired rule: a slot without a partner (``reverse[j] == -1``) gets +0.0 from all three - an edge without its transpose takes
  no part - so the result is an exactly symmetric (``out[reverse] == out`` in bits) or antisymmetric (``out[reverse] == -out``) edge
  field on every list, one-directional ones included.  Who wants another rule has ``reverse`` and ``swap``.
* The self-edge rule: a self-edge is its own partner: ``swap`` copies it, ``symmetrize`` gives ``fl32(m + m)``, ``antisymmetrize``
  gives +0.0 for a finite m (NaN for an infinite or NaN one).
* Backward: each op is its own adjoint - the two signs of ``antisymmetrize`` cancel - so the gradient of msg is the same op applied
  to the cotangent: the same kernel, the same bits.  Nothing is saved but the graph.
* bfloat16: ``round_to_bf16(float32 op(upcast))``, rounded once; ``swap`` copies the 16 bits.
* There is no fused "symmetrize, then segment_sum": as a set of terms it is ``segment_sum(msg, "receivers") + segment_sum(msg,
  "senders")``, which the library already does node-shaped.

bfloat16.  Every op takes float32 or bfloat16 tensors (what ``torch.autocast(dtype=torch.bfloat16)`` hands a module) and
returns the dtype it was given.  One contract for every op and every backward:

    the bfloat16 op  ==  round_to_bf16( the float32 op( upcast(inputs) ) )        bit for bit

upcast is the exact widening, the float32 op is the arithmetic stated above - the same order of adds, the same m, expf, s
and division - and round_to_bf16 is one round-to-nearest-even per stored element (NaN stays NaN, beyond the range +-inf,
subnormals kept, -0.0 kept where the float32 op keeps it).  So ``gather`` is a bit copy; ``segment_sum`` adds the widened
terms in float32 in slot order and rounds once - no partial sum is ever held in bfloat16, which is what ``index_add_`` on
bfloat16 (atomics on 8 significant bits, in any order) cannot give; ``segment_max`` / ``segment_min`` return one of the
inputs; ``segment_mean`` is ``(segment_sum(msg).float() / max(degree, 1)).to(bfloat16)``; ``segment_softmax`` saves the
rounded y and differentiates that.  ``attend`` on bfloat16 is NOT the composition of the bfloat16 ops: the composition rounds
the weights to bfloat16 before it multiplies, ``attend`` forms them in float32 from the widened logits and rounds the sum
once - it is the more accurate of the two; ``m`` and ``s`` stay float32.  ``conv`` on bfloat16 is NOT the composition of the
bfloat16 ops either: the composition rounds each product to bfloat16 before it adds, ``conv`` keeps the products in float32 -
exact there, 8 + 8 significant bits fit - and rounds the ordered sum once; its ``d_w`` likewise (products and the k-sum in
float32, one rounding).  ``pair_mul`` and ``pair_add`` equal torch's bfloat16 arithmetic on the gathered rows.  The engine's features stay float32, so
``torch.cat([h_bf16, features["rel_disp"]], -1)`` promotes to float32 unless the features are cast.  float16, float64 and
integer tensors are refused.

Tensors are float32 or bfloat16 on the engine's device (``TypeError`` otherwise; the logits and values of one ``attend`` the
same dtype; a cotangent in another dtype than its forward's is a ``TypeError`` too) and are made contiguous here.  A forward or a
backward after the engine's list moved on raises ``RuntimeError``: the staleness rule of ``FeatureDict``.  The ops are once
differentiable: a double backward through them (``create_graph=True``) raises.

``differentiable_features(features, window)`` gives the feature dict a ``TorchModel`` module receives as one autograd node
over the position window, so that a loss on the module's output has a gradient with respect to the positions
(``autograd.TorchModule`` uses it); its backward is one HIP launch under the same rules.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

__all__ = ["Graph", "differentiable_features"]

_ROLES = {"receivers": 0, "senders": 1}
_GATHER, _SEGMENT_SUM = 0, 1


class _Op(torch.autograd.Function):
    """gather (kind 0) or segment_sum (kind 1) over `role`; the backward is the other kind over the same role."""

    @staticmethod
    def forward(ctx, x, graph, role, kind):
        ctx.graph, ctx.role, ctx.kind, ctx.dtype = graph, role, kind, getattr(x, "dtype", None)
        return graph._run(kind, role, x)

    @staticmethod
    @once_differentiable   # (the backward runs the kernel on detached data: a double backward raises instead of giving zeros)
    def backward(ctx, d):
        return ctx.graph._run(1 - ctx.kind, ctx.role, d, ctx.dtype), None, None, None


class _SegmentMax(torch.autograd.Function):
    """segment_max / segment_min over `role`; the forward's winning slots route the gradient."""

    @staticmethod
    def forward(ctx, msg, graph, role, minimum):
        name = "segment_min" if minimum else "segment_max"
        flat, rest = graph._flat(name, msg, graph.engine.e_cap)
        out, win = graph.engine.graph_segment_max(role, flat, minimum)
        ctx.graph, ctx.role, ctx.name, ctx.rest, ctx.dtype = graph, role, name, rest, flat.dtype
        ctx.save_for_backward(win)
        return out.reshape(graph._shape(graph.engine.N) + rest)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        flat, _ = g._flat(ctx.name, d, e.N, ctx.dtype)
        d_msg = e.graph_segment_max_backward(ctx.role, flat, ctx.saved_tensors[0])
        return d_msg.reshape(g._shape(e.e_cap) + ctx.rest), None, None, None


class _SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, graph, role):
        flat, rest = graph._flat("segment_softmax", logits, graph.engine.e_cap)
        y = graph.engine.graph_segment_softmax(role, flat)
        ctx.graph, ctx.role, ctx.rest = graph, role, rest
        ctx.save_for_backward(y)
        return y.reshape(graph._shape(graph.engine.e_cap) + rest)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        flat, _ = g._flat("segment_softmax", d, e.e_cap, ctx.saved_tensors[0].dtype)
        d_x = e.graph_segment_softmax_backward(ctx.role, ctx.saved_tensors[0], flat)
        return d_x.reshape(g._shape(e.e_cap) + ctx.rest), None, None


class _Attend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, graph, role):
        e = graph.engine
        if isinstance(logits, torch.Tensor) and isinstance(values, torch.Tensor) and logits.dtype != values.dtype:
            raise TypeError(f"graph.attend: logits and values must have one dtype (float32 or bfloat16), got {logits.dtype} and "
                            f"{values.dtype}")
        lf, heads = graph._flat("attend", logits, e.e_cap)
        vf, hd = graph._flat("attend", values, e.e_cap)
        if len(heads) != 1 or len(hd) != 2 or hd[0] != heads[0]:
            raise ValueError(f"graph.attend: expected logits {graph._shape(e.e_cap) + ('H',)} and values "
                             f"{graph._shape(e.e_cap) + ('H', 'D')}, got {tuple(logits.shape)} and {tuple(values.shape)}")
        vf = vf.reshape(e.B * e.e_cap, hd[0], hd[1])
        out, m, s = e.graph_attend(role, lf, vf)
        ctx.graph, ctx.role, ctx.hd = graph, role, hd
        ctx.save_for_backward(lf, vf, m, s)
        return out.reshape(graph._shape(e.N) + hd)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        lf, vf, m, s = ctx.saved_tensors
        flat, _ = g._flat("attend", d, e.N, lf.dtype)
        d_l, d_v = e.graph_attend_backward(ctx.role, lf, vf, m, s, flat.reshape(e.B * e.N, *ctx.hd))
        return d_l.reshape(g._shape(e.e_cap) + ctx.hd[:1]), d_v.reshape(g._shape(e.e_cap) + ctx.hd), None, None


def _one_dtype(name: str, a, b, what: str) -> None:
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype != b.dtype:
        raise TypeError(f"graph.{name}: {what} must have one dtype (float32 or bfloat16), got {a.dtype} and {b.dtype}")


class _Conv(torch.autograd.Function):
    """conv over `role`: d_x is conv of the cotangent over the other role, d_w the K-reducing pair_mul of x and the cotangent."""

    @staticmethod
    def forward(ctx, x, w, graph, role):
        e = graph.engine
        _one_dtype("conv", x, w, "x and w")
        xf, rx = graph._flat("conv", x, e.N)
        wf, rw = graph._flat("conv", w, e.e_cap)
        if rx == rw:                                       # trailing dimensions fold into C
            K = 1
        elif len(rw) == 1 and len(rx) == 2 and rx[1] == rw[0]:
            K = rx[0]                                      # w is broadcast over the K rows of a node
        else:
            raise ValueError(f"graph.conv: expected x {graph._shape(e.N) + ('C',)} or {graph._shape(e.N) + ('K', 'C')} and w "
                             f"{graph._shape(e.e_cap) + ('C',)} (or equal trailing dimensions), got {tuple(x.shape)} and "
                             f"{tuple(w.shape)}")
        xf = xf.reshape(e.B * e.N, K, -1)
        out = e.graph_conv(role, xf, wf)
        ctx.graph, ctx.role, ctx.rx, ctx.rw = graph, role, rx, rw
        ctx.save_for_backward(xf, wf)
        return out.reshape(graph._shape(e.N) + rx)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        xf, wf = ctx.saved_tensors
        df, _ = g._flat("conv", d, e.N, xf.dtype)
        df = df.reshape(xf.shape)
        d_x = d_w = None
        if ctx.needs_input_grad[0]:
            d_x = e.graph_conv(1 - ctx.role, df, wf).reshape(g._shape(e.N) + ctx.rx)
        if ctx.needs_input_grad[1]:
            d_w = e.graph_pair_mul(1 - ctx.role, xf, df).reshape(g._shape(e.e_cap) + ctx.rw)
        return d_x, d_w, None, None


class _Pair(torch.autograd.Function):
    """pair_mul / pair_add: a over senders, b over receivers."""

    @staticmethod
    def forward(ctx, a, b, graph, mul):
        e = graph.engine
        name = "pair_mul" if mul else "pair_add"
        _one_dtype(name, a, b, "a and b")
        af, ra = graph._flat(name, a, e.N)
        bf, rb = graph._flat(name, b, e.N)
        if ra != rb:
            raise ValueError(f"graph.{name}: a and b must have one shape {graph._shape(e.N) + ('C',)}, got {tuple(a.shape)} and "
                             f"{tuple(b.shape)}")
        ctx.graph, ctx.mul, ctx.rest, ctx.dtype = graph, mul, ra, af.dtype
        if mul:
            ctx.save_for_backward(af, bf)
            out = e.graph_pair_mul(_ROLES["senders"], af[:, None, :], bf[:, None, :])
        else:
            out = e.graph_pair_add(_ROLES["senders"], af, bf)
        return out.reshape(graph._shape(e.e_cap) + ra)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        df, _ = g._flat("pair_mul" if ctx.mul else "pair_add", d, e.e_cap, ctx.dtype)
        grads = [None, None]
        for k, role in enumerate((_ROLES["senders"], _ROLES["receivers"])):
            if not ctx.needs_input_grad[k]:
                continue
            if ctx.mul:   # d_a = conv(b, d, senders), d_b = conv(a, d, receivers)
                out = e.graph_conv(role, ctx.saved_tensors[1 - k][:, None, :], df)
            else:
                out = e.graph_segment_sum(role, df)
            grads[k] = out.reshape(g._shape(e.N) + ctx.rest)
        return grads[0], grads[1], None, None


_SWAP, _SYM, _ANTISYM = 0, 1, 2   # LB_GRAPH_PAIR_* (include/lbhip.h)
_PAIR_NAMES = ("swap", "symmetrize", "antisymmetrize")


class _EdgePair(torch.autograd.Function):
    """swap / symmetrize / antisymmetrize: each is its own adjoint, so the backward is the forward on the cotangent.  Nothing is
    saved but the graph."""

    @staticmethod
    def forward(ctx, msg, graph, mode):
        e = graph.engine
        flat, rest = graph._flat(_PAIR_NAMES[mode], msg, e.e_cap)
        ctx.graph, ctx.mode, ctx.dtype = graph, mode, flat.dtype
        return e.graph_edge_pair(mode, flat).reshape(graph._shape(e.e_cap) + rest)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        flat, rest = g._flat(_PAIR_NAMES[ctx.mode], d, e.e_cap, ctx.dtype)
        return e.graph_edge_pair(ctx.mode, flat).reshape(g._shape(e.e_cap) + rest), None, None


_MAX_K = 9   # LB_GRAPH_MAX_K (csrc/lb_graph.hip): u rows are read as scalars into registers


def _vec_args(graph, name: str, node, w, u, vector: bool):
    """The checks of conv_vec (node = x (B, N, C)) and conv_dot (node = v (B, N, K, C)) -> the flat node tensor ((B N, C) or
    (B N, K, C)), w (B E_cap, C), u (B E_cap, K)."""
    e = graph.engine
    _one_dtype(name, node, w, "x, w and u" if not vector else "v, w and u")
    _one_dtype(name, w, u, "x, w and u" if not vector else "v, w and u")
    nf, rn = graph._flat(name, node, e.N)
    wf, rw = graph._flat(name, w, e.e_cap)
    uf, ru = graph._flat(name, u, e.e_cap)
    if len(rw) != 1 or len(ru) != 1 or rn != ((ru + rw) if vector else rw) or not 1 <= ru[0] <= _MAX_K:
        raise ValueError(f"graph.{name}: expected {'v' if vector else 'x'} {graph._shape(e.N) + (('K', 'C') if vector else ('C',))}, "
                         f"w {graph._shape(e.e_cap) + ('C',)} and u {graph._shape(e.e_cap) + ('K',)} with 1 <= K <= {_MAX_K}, got "
                         f"{tuple(node.shape)}, {tuple(w.shape)} and {tuple(u.shape)}")
    return (nf.reshape(e.B * e.N, ru[0], rw[0]) if vector else nf), wf, uf


class _ConvVec(torch.autograd.Function):
    """conv_vec over `role`: d_x is conv_dot of the cotangent over the other role; d_w and d_u come from one edge launch with
    S = x at the slot's other node and V = the cotangent at its `role` node."""

    @staticmethod
    def forward(ctx, x, w, u, graph, role):
        e = graph.engine
        xf, wf, uf = _vec_args(graph, "conv_vec", x, w, u, False)
        out = e.graph_conv_vec(role, xf, wf, uf)
        ctx.graph, ctx.role = graph, role
        ctx.save_for_backward(xf, wf, uf)
        return out.reshape(graph._shape(e.N) + (uf.shape[1], wf.shape[1]))

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        xf, wf, uf = ctx.saved_tensors
        df, _ = g._flat("conv_vec", d, e.N, xf.dtype)
        df = df.reshape(e.B * e.N, uf.shape[1], wf.shape[1])
        need = ctx.needs_input_grad
        d_x = d_w = d_u = None
        if need[0]:
            d_x = e.graph_conv_dot(1 - ctx.role, df, wf, uf).reshape(g._shape(e.N) + (wf.shape[1],))
        if need[1] or need[2]:
            d_w, d_u = e.graph_conv_vec_edge_grad(1 - ctx.role, xf, df, wf, uf, need[1], need[2])
            d_w = None if d_w is None else d_w.reshape(g._shape(e.e_cap) + (wf.shape[1],))
            d_u = None if d_u is None else d_u.reshape(g._shape(e.e_cap) + (uf.shape[1],))
        return d_x, d_w, d_u, None, None


class _ConvDot(torch.autograd.Function):
    """conv_dot over `role`: d_v is conv_vec of the cotangent over the other role; d_w and d_u come from one edge launch with
    S = the cotangent at the slot's `role` node and V = v at its other node."""

    @staticmethod
    def forward(ctx, v, w, u, graph, role):
        e = graph.engine
        vf, wf, uf = _vec_args(graph, "conv_dot", v, w, u, True)
        out = e.graph_conv_dot(role, vf, wf, uf)
        ctx.graph, ctx.role = graph, role
        ctx.save_for_backward(vf, wf, uf)
        return out.reshape(graph._shape(e.N) + (wf.shape[1],))

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        vf, wf, uf = ctx.saved_tensors
        df, _ = g._flat("conv_dot", d, e.N, vf.dtype)
        need = ctx.needs_input_grad
        d_v = d_w = d_u = None
        if need[0]:
            d_v = e.graph_conv_vec(1 - ctx.role, df, wf, uf).reshape(g._shape(e.N) + (uf.shape[1], wf.shape[1]))
        if need[1] or need[2]:
            d_w, d_u = e.graph_conv_vec_edge_grad(ctx.role, df, vf, wf, uf, need[1], need[2])
            d_w = None if d_w is None else d_w.reshape(g._shape(e.e_cap) + (wf.shape[1],))
            d_u = None if d_u is None else d_u.reshape(g._shape(e.e_cap) + (uf.shape[1],))
        return d_v, d_w, d_u, None, None


_MAX_R = 32   # LB_GRAPH_MAX_R (include/lbhip.h): the weight columns of a unit live in registers


class _FilterConv(torch.autograd.Function):
    """filter_conv over `role`: d_x is filter_conv of the cotangent over the other role; d_f and d_weight come from the edge
    launches of graph_filter_conv_grad.  Only x, f and weight are saved."""

    @staticmethod
    def forward(ctx, x, f, weight, graph, role):
        e = graph.engine
        _one_dtype("filter_conv", x, f, "x, f and weight")
        _one_dtype("filter_conv", x, weight, "x, f and weight")
        xf, rx = graph._flat("filter_conv", x, e.N)
        ff, rf = graph._flat("filter_conv", f, e.e_cap)
        ok = (isinstance(weight, torch.Tensor) and weight.dim() == 2 and len(rf) == 1 and len(rx) in (1, 2)
              and tuple(weight.shape) == (rf[0], rx[-1]) and 1 <= rf[0] <= _MAX_R)
        if not ok:
            raise ValueError(f"graph.filter_conv: expected x {graph._shape(e.N) + ('C',)} or {graph._shape(e.N) + ('K', 'C')}, f "
                             f"{graph._shape(e.e_cap) + ('R',)} and weight ('R', 'C') with 1 <= R <= {_MAX_R}, got {tuple(x.shape)}, "
                             f"{tuple(f.shape)} and {tuple(getattr(weight, 'shape', ()))}")
        if weight.device != e.device:
            raise TypeError(f"graph.filter_conv: weight is on {weight.device}, the engine on {e.device}")
        wt = weight.detach().contiguous()
        xf = xf.reshape(e.B * e.N, -1, rx[-1])
        out = e.graph_filter_conv(role, xf, ff, wt)
        ctx.graph, ctx.role, ctx.rx = graph, role, rx
        ctx.save_for_backward(xf, ff, wt)
        return out.reshape(graph._shape(e.N) + rx)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        xf, ff, wt = ctx.saved_tensors
        df, _ = g._flat("filter_conv", d, e.N, xf.dtype)
        df = df.reshape(xf.shape)
        need = ctx.needs_input_grad
        d_x = d_f = d_weight = None
        if need[0]:
            d_x = e.graph_filter_conv(1 - ctx.role, df, ff, wt).reshape(g._shape(e.N) + ctx.rx)
        if need[1] or need[2]:
            d_f, d_weight = e.graph_filter_conv_grad(ctx.role, xf, df, ff, wt, need[1], need[2])
            d_f = None if d_f is None else d_f.reshape(g._shape(e.e_cap) + (ff.shape[1],))
        return d_x, d_f, d_weight, None, None


_AGG_CODES = {"sum": 1, "mean": 2, "max": 3, "min": 4, "std": 5, "var": 6}   # LB_AGG_* (include/lbhip.h)


def _agg_word(name: str, ops, eps) -> tuple:
    """The checks of aggregate's `ops` and `eps` -> (the names as a tuple, the ops word: one nibble per plane from the low end)."""
    names = (ops,) if isinstance(ops, str) else tuple(ops)
    if not names:
        raise ValueError(f"graph.{name}: ops is empty; expected some of {tuple(_AGG_CODES)}")
    word = 0
    for a, op in enumerate(names):
        if op not in _AGG_CODES:
            raise ValueError(f"graph.{name}: unknown op {op!r}; expected some of {tuple(_AGG_CODES)}")
        if op in names[:a]:
            raise ValueError(f"graph.{name}: op {op!r} is named twice in {names}")
        word |= _AGG_CODES[op] << (4 * a)
    if "std" in names and not float(eps) > 0.0:
        raise ValueError(f"graph.{name}: eps must be > 0 with 'std', got {eps!r}")
    return names, word


class _Aggregate(torch.autograd.Function):
    """aggregate over `role`: one node-parallel launch forward, one edge-parallel launch backward.  The winning slots and the
    float32 mean and std come back from the forward; msg is saved only when std or var needs the centred values again."""

    @staticmethod
    def forward(ctx, msg, graph, role, names, word, eps):
        e = graph.engine
        flat, rest = graph._flat("aggregate", msg, e.e_cap)
        out, win, stats = e.graph_aggregate(role, flat, word, eps, len(names))
        ctx.graph, ctx.role, ctx.word, ctx.planes, ctx.rest, ctx.dtype = graph, role, word, len(names), rest, flat.dtype
        ctx.save_for_backward(flat if stats is not None else None, win, stats)
        return out.reshape(graph._shape(e.N) + (len(names),) + rest)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g, e = ctx.graph, ctx.graph.engine
        msg, win, stats = ctx.saved_tensors
        flat, _ = g._flat("aggregate", d, e.N, ctx.dtype)
        d_msg = e.graph_aggregate_backward(ctx.role, flat.reshape(e.B * e.N, ctx.planes, -1), msg, win, stats, ctx.word)
        return d_msg.reshape(g._shape(e.e_cap) + ctx.rest), None, None, None, None, None


_FLOAT_KEYS = ("abs_pos", "vel_hist", "vel_mag", "bound", "force", "rel_disp", "rel_dist")
_GRAD_KEYS = ("abs_pos", "vel_hist", "vel_mag", "bound", "rel_disp", "rel_dist")   # ("force" is a constant of the positions)


def _plain(features, key: str) -> torch.Tensor:
    """One value of a FeatureDict as a TorchModel module receives it: batched, float32 (indices int64)."""
    v = features[key]
    v = v if features.batched else v[None]
    return v.to(torch.int64 if key in ("senders", "receivers") else torch.float32)


class _Features(torch.autograd.Function):
    """The float features of a FeatureDict as functions of the window; the backward is one lb_graph_features_backward."""

    @staticmethod
    def forward(ctx, window, features, keys):
        ctx.features, ctx.keys = features, keys
        outs = [_plain(features, k) for k in keys]
        ctx.mark_non_differentiable(*[o for k, o in zip(keys, outs) if k not in _GRAD_KEYS])
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        f, e = ctx.features, ctx.features.engine
        if e.version != f.version:
            raise RuntimeError("graph.differentiable_features: the engine's neighbor list changed since these features were "
                               "produced (features are stale)")
        rows = {"rel_disp": e.B * e.e_cap, "rel_dist": e.B * e.e_cap}
        args = {}
        for k, g in zip(ctx.keys, grads):
            if g is None or k not in _GRAD_KEYS:
                continue
            if g.dtype != torch.float32 or g.device != e.device:
                raise TypeError(f"graph.differentiable_features: the gradient of {k!r} is {g.dtype} on {g.device}, expected "
                                f"float32 on {e.device}")
            g = g.detach().contiguous()
            args["d_" + k] = g.reshape((rows.get(k, e.B * e.N),) + tuple(g.shape[2:]))
        return e.graph_features_backward(**args), None, None


def differentiable_features(features, window: torch.Tensor) -> dict:
    """The plain batched dict a ``TorchModel`` module receives - the float keys as float32 with the bits of
    ``features[k].to(torch.float32)``, ``senders`` / ``receivers`` as int64 - with the float keys as ONE autograd node over
    `window` ((B, N, isl, dim) float64: the window `features` describes).  Its backward is one HIP launch
    (``lb_graph_features_backward``): the transpose of the feature builder on the engine's current window and list - velocity
    history and magnitudes, wall distances, relative displacements and distances; the neighbor list is held fixed and
    ``force`` carries no gradient.  Once differentiable; a backward after the engine moved on raises ``RuntimeError``."""
    engine = getattr(features, "engine", None)
    if engine is None:
        raise TypeError("graph.differentiable_features needs the FeatureDict returned by case.preprocess* / allocate* (it "
                        "names the engine and the list to run on)")
    if engine.geometry_f32:
        raise NotImplementedError("graph.differentiable_features: the window gradient is built for float64 geometry only "
                                  "(the case was made with dtype=float32)")
    shape = (engine.B, engine.N, engine.isl, engine.dim)
    if not isinstance(window, torch.Tensor) or tuple(window.shape) != shape or window.dtype != torch.float64:
        raise ValueError(f"graph.differentiable_features: window must be {shape} float64, got "
                         f"{tuple(getattr(window, 'shape', ()))} {getattr(window, 'dtype', type(window))}")
    if window.device != engine.device:
        raise TypeError(f"graph.differentiable_features: the window is on {window.device}, the engine on {engine.device}")
    if engine.version != features.version:
        raise RuntimeError("graph.differentiable_features: the engine's neighbor list changed since these features were "
                           "produced (features are stale)")
    keys = tuple(k for k in features.keys() if k in _FLOAT_KEYS)
    out = dict(zip(keys, _Features.apply(window, features, keys)))
    return {k: out[k] if k in out else _plain(features, k) for k in features.keys()}


class Graph:
    """The engine's current list behind `features` (a FeatureDict), as differentiable gather / segment_sum and the attention
    ops (degree, segment_mean / max / min / softmax, attend), the multi-aggregator (aggregate, segment_std / var) and the edge messages (conv, pair_mul, pair_add, conv_vec,
    conv_dot, filter_conv), and the edge pairs (reverse, swap, symmetrize, antisymmetrize).
    `batched`: whether the tensors carry the leading B (default: as the features do)."""

    def __init__(self, features, batched: Optional[bool] = None):
        engine = getattr(features, "engine", None)
        if engine is None:
            raise TypeError("graph.Graph needs the FeatureDict returned by case.preprocess* / allocate* (it names the "
                            "engine and the list to run on)")
        self.features, self.engine, self.version = features, engine, features.version
        self.batched = bool(features.batched if batched is None else batched)
        if not self.batched and engine.B != 1:
            raise ValueError(f"graph.Graph: un-batched tensors on an engine of batch {engine.B}")
        self._idx = None
        self._rev = None

    # ------------------------------------------------------------------ the list
    def _check_fresh(self, what: str) -> None:
        if self.engine.version != self.version:
            raise RuntimeError(f"graph.{what}: the engine's neighbor list changed since these features were produced "
                               "(features are stale)")

    def _export(self):
        if self._idx is None:
            self._check_fresh("Graph")
            self._idx = self.engine.nl_idx()
        return self._idx

    def _lead(self, t: torch.Tensor) -> torch.Tensor:
        return t if self.batched else t[0]

    @property
    def n_edges(self) -> torch.Tensor:
        return self._lead(self._export()[1])

    @property
    def receivers(self) -> torch.Tensor:
        return self._lead(self._export()[0][:, 0])

    @property
    def senders(self) -> torch.Tensor:
        return self._lead(self._export()[0][:, 1])

    @property
    def reverse(self) -> torch.Tensor:
        """(B, E_cap) int32: for the real slot of (receiver r, sender s) the slot, within its trajectory, of the edge (receiver s,
        sender r); a self-edge maps to itself; -1 where the list holds no such edge (an edge in one direction only) and in every
        pad slot.  reverse[reverse[j]] == j wherever reverse[j] >= 0.  Built by the engine in one launch per list build; read
        once per Graph.  No autograd."""
        self._check_fresh("reverse")
        if self._rev is None:
            self._rev = self.engine.graph_reverse().reshape(self._shape(self.engine.e_cap))
        return self._rev

    # ------------------------------------------------------------------ the ops
    @staticmethod
    def _role(role) -> int:
        if role not in _ROLES:
            raise ValueError(f"role must be 'senders' or 'receivers', got {role!r}")
        return _ROLES[role]

    def _shape(self, rows: int) -> tuple:
        return (self.engine.B, rows) if self.batched else (rows,)

    def _flat(self, name: str, t: torch.Tensor, rows: int, forward_dtype=None):
        """The checks every op makes on a (B, rows, ...) tensor -> (its detached contiguous (B * rows, C) view, the trailing
        dimensions).  `forward_dtype`: t is a cotangent of a forward that ran in this dtype."""
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"graph.{name}: float32 or bfloat16 tensors only, got {getattr(t, 'dtype', type(t))}")
        if forward_dtype is not None and t.dtype != forward_dtype:
            raise TypeError(f"graph.{name}: the cotangent is {t.dtype}, the forward ran in {forward_dtype}")
        e = self.engine
        if t.device != e.device:
            raise TypeError(f"graph.{name}: the tensor is on {t.device}, the engine on {e.device}")
        self._check_fresh(name)
        lead = self._shape(rows)
        if tuple(t.shape[:len(lead)]) != lead or t.dim() <= len(lead) or t.numel() == 0:
            raise ValueError(f"graph.{name}: expected {lead + ('C',)} (C >= 1), got {tuple(t.shape)}")
        return t.detach().contiguous().reshape(e.B * rows, -1), tuple(t.shape[len(lead):])

    def _run(self, kind: int, role: int, t: torch.Tensor, forward_dtype=None) -> torch.Tensor:
        e = self.engine
        flat, rest = self._flat("segment_sum" if kind == _SEGMENT_SUM else "gather", t, e.e_cap if kind == _SEGMENT_SUM else e.N,
                                forward_dtype)
        out = (e.graph_segment_sum if kind == _SEGMENT_SUM else e.graph_gather)(role, flat)
        return out.reshape(self._shape(e.N if kind == _SEGMENT_SUM else e.e_cap) + rest)

    def gather(self, x: torch.Tensor, role: str) -> torch.Tensor:
        """x (B, N, C) -> (B, E_cap, C): x[b, role index of slot (b, j)] in the real slots, +0.0 in the pad slots."""
        return _Op.apply(x, self, self._role(role), _GATHER)

    def segment_sum(self, msg: torch.Tensor, role: str) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, C): per node the ordered float32 sum of the real slots whose role index it is; for
        bfloat16 the terms are widened and that float32 sum is rounded once."""
        return _Op.apply(msg, self, self._role(role), _SEGMENT_SUM)

    def degree(self, role: str) -> torch.Tensor:
        """-> (B, N) int32: the number of real slots whose role index is the node.  No autograd."""
        r = self._role(role)
        self._check_fresh("degree")
        return self.engine.graph_degree(r).reshape(self._shape(self.engine.N))

    def segment_mean(self, msg: torch.Tensor, role: str) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, C): segment_sum divided by max(degree, 1) as float32 - the ordered sum, then one
        correctly rounded division; +0.0 for a node without edges.  bfloat16: the rounded ordered sum, widened, one float32
        division, one rounding."""
        total = self.segment_sum(msg, role)
        deg = self.degree(role).clamp(min=1).to(torch.float32)
        return (total.float() / deg.reshape(deg.shape + (1,) * (total.dim() - deg.dim()))).to(total.dtype)

    def segment_max(self, msg: torch.Tensor, role: str) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, C): per node and column the first real slot's value, replaced in ascending slot order
        only by a strictly greater one (ties keep the earlier slot; a NaN wins and stays).  A node without edges gets +0.0
        where jraph gives -inf, as segment_sum does, so that it feeds finite values onward.  The gradient goes to the
        winning slot; every other slot of it, pads included, is +0.0."""
        return _SegmentMax.apply(msg, self, self._role(role), False)

    def segment_min(self, msg: torch.Tensor, role: str) -> torch.Tensor:
        """segment_max with "strictly smaller"; a node without edges gets +0.0 (jraph: +inf)."""
        return _SegmentMax.apply(msg, self, self._role(role), True)

    def aggregate(self, msg: torch.Tensor, role: str, ops=("sum", "mean", "max", "min", "std"), eps: float = 1e-5) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, A, C), A = len(ops): the named reductions of msg over each node's real slots of `role`,
        in the order of `ops` - distinct names out of sum, mean, max, min, std, var - from ONE launch that walks the row once
        (twice with std / var, for the centred squares) and ONE launch backward.  sum, mean, max and min have the bits of
        segment_sum, segment_mean, segment_max and segment_min; var is the centred two-pass population variance, std is
        sqrt(var + eps); a node without slots gets +0.0 in every plane.  The module docstring states every rounding."""
        names, word = _agg_word("aggregate", ops, eps)
        return _Aggregate.apply(msg, self, self._role(role), names, word, float(eps))

    def segment_std(self, msg: torch.Tensor, role: str, eps: float = 1e-5) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, C): aggregate(msg, role, ("std",), eps) without the plane axis - sqrt(var + eps) of the
        node's real slots, +0.0 for a node without slots."""
        names, word = _agg_word("segment_std", ("std",), eps)
        return _Aggregate.apply(msg, self, self._role(role), names, word, float(eps)).select(self._plane, 0)

    def segment_var(self, msg: torch.Tensor, role: str) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, N, C): aggregate(msg, role, ("var",)) without the plane axis - the centred two-pass
        population variance of the node's real slots."""
        names, word = _agg_word("segment_var", ("var",), 1.0)
        return _Aggregate.apply(msg, self, self._role(role), names, word, 1.0).select(self._plane, 0)

    @property
    def _plane(self) -> int:
        return 2 if self.batched else 1   # the axis of aggregate's planes

    def segment_softmax(self, logits: torch.Tensor, role: str) -> torch.Tensor:
        """logits (B, E_cap, C) -> (B, E_cap, C): one softmax per node and column over the node's real slots, shifted by
        their maximum, the denominator summed in ascending slot order; +0.0 in the pad slots."""
        return _SegmentSoftmax.apply(logits, self, self._role(role))

    def attend(self, logits: torch.Tensor, values: torch.Tensor, role: str) -> torch.Tensor:
        """logits (B, E_cap, H), values (B, E_cap, H, D) -> (B, N, H, D): bit for bit
        segment_sum(segment_softmax(logits, role)[..., None] * values, role), in one kernel that reads the values once and
        writes nothing of their size.  On bfloat16 (logits and values alike) it is that float32 result on the widened inputs,
        rounded once: not the composition of the bfloat16 ops, which rounds the weights to bfloat16 first, and the more
        accurate of the two."""
        return _Attend.apply(logits, values, self, self._role(role))

    def conv(self, x: torch.Tensor, w: torch.Tensor, role: str) -> torch.Tensor:
        """x (B, N, C) or (B, N, K, C), w (B, E_cap, C) -> the shape of x: per node the ordered sum over its real slots of
        `role` of x[the slot's other node] * w[slot] (w broadcast over K) - bit for bit
        segment_sum(gather(x, other role) * w[..., None, :], role) on float32, in one kernel that reads w once and writes
        nothing edge-shaped.  Equal trailing dimensions fold into C.  On bfloat16 the exact products are summed in float32 and
        the sum is rounded once: not the composition of the bfloat16 ops, which rounds every product first."""
        return _Conv.apply(x, w, self, self._role(role))

    def filter_conv(self, x: torch.Tensor, f: torch.Tensor, weight: torch.Tensor, role: str) -> torch.Tensor:
        """x (B, N, C) or (B, N, K, C), f (B, E_cap, R) with 1 <= R <= 32, weight (R, C) -> the shape of x: conv(x, wf, role) with
        the continuous filter wf = f @ weight formed in registers - wf[j, c] = f[j, 0] * weight[0, c] + f[j, 1] * weight[1, c] +
        ..., r ascending, every product rounded to float32, the first starts the sum (not torch's matmul, whose order is
        unstated) - so that nothing edge-shaped of C columns exists, forward or backward.  f is any per-edge basis (Gaussians of
        rel_dist times a cutoff); its pad slots may hold NaN.  There is no bias argument: a bias is a column of f - ones, or the
        cutoff envelope, since (Linear(rbf) + b) * fcut = [rbf * fcut, fcut] @ [W; b].  On float32 bit for bit conv on that wf;
        on bfloat16 the float32 result on the widened inputs, rounded once, d_f and d_weight included.  A float32 weight beside
        bfloat16 x and f (a Parameter under autocast) is cast to bfloat16 first; its gradient arrives in float32.  The module
        docstring states the order of every gradient sum."""
        if (isinstance(weight, torch.Tensor) and isinstance(x, torch.Tensor) and isinstance(f, torch.Tensor)
                and weight.dtype == torch.float32 and x.dtype == f.dtype == torch.bfloat16):
            weight = weight.to(x.dtype)                    # differentiable: what autocast does to a Linear's weight
        return _FilterConv.apply(x, f, weight, self, self._role(role))

    def conv_vec(self, x: torch.Tensor, w: torch.Tensor, u: torch.Tensor, role: str) -> torch.Tensor:
        """x (B, N, C), w (B, E_cap, C), u (B, E_cap, K) with 1 <= K <= 9 -> (B, N, K, C), scalar to vector channels: per node
        the ordered sum over its real slots of `role` of (x[the slot's other node] * w[slot]) * u[slot, k] - PaiNN's
        ``w_vs s_j (x) r_ij``, EGNN's position update at C = 1 - bit for bit
        segment_sum((gather(x, other role) * w)[..., None, :] * u[..., :, None], role) on float32, in one kernel that writes
        nothing edge-shaped.  On bfloat16 the float32 result on the widened inputs, rounded once."""
        return _ConvVec.apply(x, w, u, self, self._role(role))

    def conv_dot(self, v: torch.Tensor, w: torch.Tensor, u: torch.Tensor, role: str) -> torch.Tensor:
        """v (B, N, K, C), w (B, E_cap, C), u (B, E_cap, K) with 1 <= K <= 9 -> (B, N, C), vector to scalar channels: per node
        the ordered sum over its real slots of `role` of w[slot] * <v[the slot's other node], u[slot]>, the inner product added
        k by k from its first product - bit for bit segment_sum(w * t, role) on float32 with t spelled out from
        gather(v, other role)[..., k, :] * u[..., k:k+1].  The adjoint of conv_vec over the other role."""
        return _ConvDot.apply(v, w, u, self, self._role(role))

    def pair_mul(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a, b (B, N, C) -> (B, E_cap, C): a[senders] * b[receivers] in the real slots (one rounded product), +0.0 in the
        pad slots; neither gathered tensor exists."""
        return _Pair.apply(a, b, self, True)

    def pair_add(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a, b (B, N, C) -> (B, E_cap, C): a[senders] + b[receivers] in the real slots, +0.0 in the pad slots - the edge
        Linear of cat[x_s, x_r, e] as (x W_s)[senders] + (x W_r)[receivers] + e W_e, with the GEMMs on N rows."""
        return _Pair.apply(a, b, self, False)

    def swap(self, msg: torch.Tensor) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, E_cap, C): msg[reverse[j]] in slot j, a bit copy - what the opposite edge holds.  +0.0 in a
        slot without a partner and in the pad slots.  Its own adjoint: the backward is swap of the cotangent."""
        return _EdgePair.apply(msg, self, _SWAP)

    def symmetrize(self, msg: torch.Tensor) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, E_cap, C): fl32(msg[j] + msg[reverse[j]]), so that out[reverse] == out bit for bit.  A slot
        whose edge has no transpose in the list gets +0.0 - it takes no part, which keeps the field exactly symmetric on a list
        with one-directional edges; another rule can be written with `reverse` and `swap`.  A self-edge gives fl32(m + m).  Pad
        slots are +0.0 and never read.  bfloat16: the float32 sum of the widened values, rounded once.  Its own adjoint.  There is
        no fused symmetrize-then-segment_sum: as a set of terms it is segment_sum(msg, "receivers") + segment_sum(msg, "senders")."""
        return _EdgePair.apply(msg, self, _SYM)

    def antisymmetrize(self, msg: torch.Tensor) -> torch.Tensor:
        """msg (B, E_cap, C) -> (B, E_cap, C): fl32(msg[j] - msg[reverse[j]]), so that out[reverse] == -out exactly - a pairwise
        force with F_ij = -F_ji, whose segment_sum over receivers conserves linear momentum up to the rounding of the row sums.
        A slot whose edge has no transpose in the list gets +0.0 (it takes no part; see symmetrize), and so does a self-edge
        with a finite value.  Pad slots are +0.0 and never read.  Its own adjoint: the backward is antisymmetrize of the
        cotangent."""
        return _EdgePair.apply(msg, self, _ANTISYM)
