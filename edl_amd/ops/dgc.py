"""DGC top-k compress / decode over one flat fp32 bucket.

    payload = dgc_compress(g, u, v, p, mu, wd, k)   # int32 [2, k]
    dgc_decode(out, [payload_rank0, payload_rank1, ...])

dgc_compress does, in place,

    u = mu*u + (g + wd*p)        (p=None: no weight-decay term)
    v = v + u
    select on |v|; payload = the (index, v[index]) pairs; v[sel] = u[sel] = 0

Selection rule — deterministic, independent of thread order, the same in
both paths. a_i = the bit pattern of |v_i| as an unsigned 31-bit integer
(non-finite values therefore sort highest), P = the k-th largest a_i.
Select {a_i >= P} if count(a >= P) <= k, else {a_i > P}; never a_i == 0.
So nsel <= k always, and the set is torch.topk's whenever no tie crosses
the boundary.

Payload: int32 [2, k]; row 0 = indices (-1 = empty slot), row 1 = the
fp32 bits (0 in an empty slot). The order of the slots is unspecified.

dgc_decode zeroes `out` and adds the payloads in list order, one pass
each. Indices are unique within a payload, so a pass is a plain
read-add-write: every caller that decodes the same list performs the same
fp32 additions in the same order and gets the same bits.

CUDA tensors run the HIP kernels (csrc/dgc.hip; nothing reads back to the
host); CPU tensors run the torch path, which is also the tests' reference.
"""
import torch

from . import ext

# pass-0 LDS histogram copies (csrc/dgc.hip); docs/kernels.md has the
# 1-copy / 4-copy timing
HIST_COPIES = 4

_WS = {}


def _workspace(device):
    """Per-device select workspace: zeroed once, the kernels leave it
    clean. Calls on one device must be stream-ordered."""
    ws = _WS.get(device)
    if ws is None:
        ws = torch.zeros(ext().dgc_workspace_words(), dtype=torch.int32,
                         device=device)
        _WS[device] = ws
    return ws


def _check(g, u, v, p, k):
    n = v.numel()
    for name, t in (("g", g), ("u", u), ("v", v), ("p", p)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("dgc: %s must be a flat contiguous fp32 tensor"
                             % name)
        if t.numel() != n or t.device != v.device:
            raise ValueError("dgc: %s does not match v" % name)
    if not 1 <= n < 2 ** 31:
        raise ValueError("dgc: 1 <= n < 2^31 required")
    if not 1 <= k <= n:
        raise ValueError("dgc: 1 <= k <= n required, got k=%d n=%d" % (k, n))


def select_threshold(v, k):
    """The rule's threshold T as an int64 scalar tensor: the selected set
    is {a_i >= T} with a = abs_bits(v). Torch path only."""
    a = abs_bits(v)
    n = a.numel()
    P = torch.kthvalue(a, n - k + 1).values  # the k-th largest
    T = torch.where((a >= P).sum() <= k, P, P + 1)
    return T.clamp(min=1)


def abs_bits(v):
    return (v.view(torch.int32) & 0x7FFFFFFF).to(torch.int64)


def _compress_torch(g, u, v, p, mu, wd, k):
    t = g if p is None else g + wd * p
    u.mul_(mu).add_(t)
    v.add_(u)
    sel = (abs_bits(v) >= select_threshold(v, k)).nonzero().view(-1)
    nsel = sel.numel()
    payload = torch.zeros(2, k, dtype=torch.int32, device=v.device)
    payload[0, nsel:] = -1
    payload[0, :nsel] = sel.to(torch.int32)
    payload[1, :nsel] = v[sel].view(torch.int32)
    v[sel] = 0
    u[sel] = 0
    return payload


def dgc_compress(g, u, v, p, mu, wd, k, payload=None):
    """-> payload int32 [2, k] (written into `payload` when given)."""
    k = int(k)
    _check(g, u, v, p, k)
    if not v.is_cuda:
        out = _compress_torch(g, u, v, p, float(mu), float(wd), k)
        if payload is not None:
            payload.copy_(out)
            return payload
        return out
    e = ext()  # a GPU without the extension is an error, not a fallback
    if payload is None:
        payload = torch.empty(2, k, dtype=torch.int32, device=v.device)
    ws = _workspace(v.device)
    e.dgc_accumulate(g, u, v, p, float(mu), float(wd), ws, HIST_COPIES)
    e.dgc_select(v, u, payload, ws)
    return payload


def dgc_decode(out, payloads):
    """out = sum of the payloads, added in list order."""
    if out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("dgc: out must be a flat contiguous fp32 tensor")
    out.zero_()
    if out.is_cuda:
        e = ext()
        for pl in payloads:
            e.dgc_scatter_add(out, pl)
        return out
    for pl in payloads:
        keep = pl[0] >= 0
        out.index_add_(0, pl[0][keep].to(torch.int64),
                       pl[1][keep].view(torch.float32))
    return out
