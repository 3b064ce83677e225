"""Seeded inputs of the training criterion at any shape: box-shaped proposals (sigmoid of a box indicator plus noise, so that the
matching costs of different queries are well apart), 1..10 box GT masks per image, unit-norm tokens and text embeddings, labels
with ~5 % ignore pixels."""
import torch


def make_case(B, L, Q, h, w, H, W, n_cat, D, h2, w2, seed, n_range=(1, 10), device="cpu"):
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(h, dtype=torch.float32)[:, None]
    xx = torch.arange(w, dtype=torch.float32)[None, :]
    y0 = torch.rand(B, 1, Q, 1, 1, generator=g) * h * 0.6
    x0 = torch.rand(B, 1, Q, 1, 1, generator=g) * w * 0.6
    hh = torch.rand(B, 1, Q, 1, 1, generator=g) * h * 0.5 + 3
    ww = torch.rand(B, 1, Q, 1, 1, generator=g) * w * 0.5 + 3
    box = ((yy >= y0) & (yy < y0 + hh) & (xx >= x0) & (xx < x0 + ww)).float()
    props = torch.sigmoid(5.0 * (box - 0.5) + 0.8 * torch.randn(B, L, Q, h, w, generator=g))
    Y = torch.arange(H)[:, None]
    X = torch.arange(W)[None, :]
    gts = []
    for b in range(B):
        n = int(torch.randint(n_range[0], n_range[1] + 1, (1,), generator=g))
        m = torch.zeros(n, H, W, dtype=torch.uint8)
        for i in range(n):
            gy, gx = int(torch.randint(0, H * 3 // 4, (1,), generator=g)), int(torch.randint(0, W * 3 // 4, (1,), generator=g))
            gh, gw = int(torch.randint(H // 16, H // 2, (1,), generator=g)), int(torch.randint(W // 16, W // 2, (1,), generator=g))
            m[i] = ((Y >= gy) & (Y < gy + gh) & (X >= gx) & (X < gx + gw)).to(torch.uint8)
        gts.append(m)
    tok = torch.randn(B, h2, w2, D, generator=g)
    tok = tok / tok.norm(dim=-1, keepdim=True)
    te = torch.randn(n_cat, D, generator=g)
    te = te / te.norm(dim=-1, keepdim=True)
    sem = torch.randint(0, n_cat, (B, H, W), generator=g)
    sem[torch.rand(B, H, W, generator=g) < 0.05] = 255
    return props.to(device), gts, tok.to(device), te.to(device), sem
