"""The CPU reference of ``dagl_graph_refresh``'s candidates and selection, in plain torch (checked against brute force by
test_graph_refresh_reference.py before any GPU test relies on it).

Dense form: a row's candidate set and its selection are bool masks [rows, N] over the keys of the row's own image."""
import torch


def candidate_mask(row_off, key, H, W, radius):
    """[rows, N] bool: key j is a candidate of row r iff it lies in the (2 radius + 1)^2 window, clipped at the map border, of some edge
    of r whose key is in [0, N).  Repeats and overlaps count once; keys outside [0, N) contribute nothing."""
    N = H * W
    n_rows = row_off.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n_rows), row_off[1:] - row_off[:-1])
    key = key.long()
    valid = (key >= 0) & (key < N)
    rows, key = rows[valid], key[valid]
    d = torch.arange(-radius, radius + 1)
    ny = (torch.div(key, W, rounding_mode="floor").view(-1, 1, 1) + d.view(1, -1, 1)).expand(-1, -1, d.numel())
    nx = ((key % W).view(-1, 1, 1) + d.view(1, 1, -1)).expand(-1, d.numel(), -1)
    inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
    r = rows.view(-1, 1, 1).expand_as(ny)[inside]
    mask = torch.zeros(n_rows, N, dtype=torch.bool)
    mask[r, (ny * W + nx)[inside]] = True
    return mask


def select_mask(cand, S, tau=None, k=0):
    """[rows, N] bool: the selection rule applied to the candidates ``cand`` [rows, N] with scores ``S`` [rows, N] (compared in S's own
    dtype; entries off the candidates are not looked at).  With ``tau`` [rows] a candidate passes iff S - tau > 0, without it all pass;
    with k > 0 the min(k, passing) passing candidates with the largest S stay, a tie at the last place going to the lower key."""
    passing = cand.clone()
    if tau is not None:
        passing &= (S - tau.to(S.dtype).view(-1, 1)) > 0
    if k <= 0:
        return passing
    low = torch.finfo(S.dtype).min
    ranked = torch.where(passing, S, torch.full_like(S, low))
    # a stable descending sort: among equal scores the lower key comes first
    order = torch.sort(ranked, dim=1, descending=True, stable=True).indices[:, :k]
    keep = torch.zeros_like(passing)
    keep.scatter_(1, order, True)
    return keep & passing


def csr_of(mask):
    """(row_off [rows + 1] int64, key [E] int32) of a [rows, N] bool mask, keys ascending inside a row."""
    deg = mask.sum(dim=1)
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    return row_off, mask.nonzero()[:, 1].int()


def mask_of(row_off, key, N):
    """[rows, N] bool of a CSR whose keys are all in [0, N)."""
    n_rows = row_off.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n_rows), row_off[1:] - row_off[:-1])
    mask = torch.zeros(n_rows, N, dtype=torch.bool)
    mask[rows, key.long()] = True
    return mask
