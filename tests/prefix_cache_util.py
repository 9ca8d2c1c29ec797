"""Inputs of the prompt-prefix tests (encode_prefix / generate(prefix=)), cut from shared_prefix_util.shared_case: the three images' prefix
rows, and the six queries that continue them (sample 6 of the case starts with another text: it is rejected by name, and left out)."""
import torch

from shared_prefix_util import shared_case

KEEP = [0, 1, 2, 3, 4, 5]                                          # the rows of the case that continue a prefix
TAIL_2 = 2                                                        # image 2 has one query and no share group: its prefix ends 2 tokens past the image


def prefix_case(cfg, seed=77):
    """→ shared_case(cfg, seed) plus
      pre_rows: per image the prefix ids (image 0 / 1: the group prefixes of samples 0, 2, 5 / 1, 4; image 2: sample 3's row up to 2 tokens
                past its image), pre_ids / pre_am: the same left-padded, P: their lengths;
      q_ids / q_am / q_index: the six queries (rows 0 .. 5 of the case, their padding kept) and their images, q_prefix / q_own: prefix and
                own-token counts per query, q_grid_x / q_pix_x: their expanded inputs."""
    c = dict(shared_case(cfg, seed))
    rows, n_m = c["rows"], c["n_merged"]
    p2 = rows[3].index(cfg.image_token_id) + n_m[2] + TAIL_2
    pre_rows = [rows[0][: c["prefix"][0]], rows[1][: c["prefix"][1]], rows[3][:p2]]
    Lp = max(len(r) for r in pre_rows)
    pre_ids = torch.full((3, Lp), cfg.pad_token_id, dtype=torch.long)
    pre_am = torch.zeros((3, Lp), dtype=torch.long)
    for u, r in enumerate(pre_rows):
        pre_ids[u, Lp - len(r):] = torch.tensor(r)
        pre_am[u, Lp - len(r):] = 1
    keep = torch.tensor(KEEP)
    q_index = [c["image_index"][b] for b in KEEP]
    q_prefix = [len(pre_rows[u]) for u in q_index]
    p_off = [0]
    for g in c["grid"].tolist():
        p_off.append(p_off[-1] + g[0] * g[1] * g[2])
    c.update(pre_rows=pre_rows, pre_ids=pre_ids, pre_am=pre_am, P=[len(r) for r in pre_rows], q_ids=c["ids"][keep], q_am=c["am"][keep],
             q_index=q_index, q_prefix=q_prefix, q_own=[len(rows[b]) - p for b, p in zip(KEEP, q_prefix)],
             q_grid_x=c["grid"][torch.tensor(q_index)], q_pix_x=torch.cat([c["pix"][p_off[u]: p_off[u + 1]] for u in q_index]))
    return c
