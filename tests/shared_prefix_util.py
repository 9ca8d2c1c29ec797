"""Inputs of the shared-prefix tests (generate(image_index=)): one batch of 7 queries over 3 images, and its expanded form."""
import torch

GRIDS = [[1, 8, 8], [1, 10, 12], [1, 6, 10]]
IMAGE_INDEX = [0, 1, 0, 2, 1, 0, 1]


def shared_case(cfg, seed=77):
    """→ dict(grid (3,3), pix, ids (7,L) left-padded, am, image_index, grid_x / pix_x: the expanded inputs, own: expected own-token counts,
    prefix: expected prefix length per sample (0: none)).

      image 0 (16 merged tokens): samples 0, 2, 5 — the same 6 pre tokens, then 3 more common tokens AFTER the image, then 1 / 2 / 33 own;
      image 1 (30): samples 1 and 4 share 7 pre tokens + image; sample 4's row is a strict prefix of sample 1's (P = shortest - 1: it keeps
                    one token of its own); sample 6 has a DIFFERENT pre-image text: it shares the ViT pass and no prefix;
      image 2 (15): sample 3 alone.
    Row lengths differ, so the left padding is ragged."""
    g = torch.Generator().manual_seed(seed)
    hi = min(cfg.vocab_size, cfg.image_token_id) - 1
    rnd = lambda n: torch.randint(0, hi, (n,), generator=g).tolist()
    grid = torch.tensor(GRIDS, dtype=torch.long)
    P = [int(t * h * w) for t, h, w in GRIDS]
    pix = torch.randn(sum(P), cfg.patch_dim, generator=g).to(torch.bfloat16).float()
    n_m = [p // cfg.merge_unit for p in P]
    img = lambda u: [cfg.vision_start_token_id] + [cfg.image_token_id] * n_m[u]
    pre0, common0 = rnd(5), rnd(3)
    pre1, pre1b = rnd(6), rnd(7)
    post1 = rnd(9)
    pre2 = rnd(4)

    def own(n, first):                                            # n own tokens whose first is `first`: the group's rows part exactly there
        return [first] + rnd(n - 1)
    rows = [None] * 7
    rows[0] = pre0 + img(0) + common0 + own(1, 11)
    rows[2] = pre0 + img(0) + common0 + own(2, 12)
    rows[5] = pre0 + img(0) + common0 + own(33, 13)
    rows[1] = pre1 + img(1) + post1
    rows[4] = pre1 + img(1) + post1[:5]
    rows[6] = pre1b + img(1) + rnd(4)
    rows[3] = pre2 + img(2) + rnd(8)
    L = max(len(r) for r in rows)
    ids = torch.full((7, L), cfg.pad_token_id, dtype=torch.long)
    am = torch.zeros((7, L), dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, L - len(r):] = torch.tensor(r)
        am[b, L - len(r):] = 1
    p_off = [0]
    for p in P:
        p_off.append(p_off[-1] + p)
    pix_x = torch.cat([pix[p_off[u]: p_off[u + 1]] for u in IMAGE_INDEX])
    p0 = len(pre0) + 1 + n_m[0] + 3                               # image 0's group: 3 tokens past the image
    p1 = len(rows[4]) - 1                                         # image 1's group: the shorter row keeps its last token
    prefix = [p0, p1, p0, 0, p1, p0, 0]
    return dict(grid=grid, pix=pix, ids=ids, am=am, image_index=list(IMAGE_INDEX), grid_x=grid[torch.tensor(IMAGE_INDEX)], pix_x=pix_x,
                rows=rows, prefix=prefix, own=[len(r) - p for r, p in zip(rows, prefix)], n_merged=n_m)
