"""Shared by test_stop_rules_cpu.py / test_stop_rules_gpu.py: generate(stop_sequences=, min_tokens=, max_tokens=).

Importable without a GPU:
  * the hand-written matcher cases — one table of stop sequences (SEQS), eight rows of twelve scripted tokens with their minimum and budget
    (ROWS), and what each row's end must be (finish step, reason, index), written down by hand and NOT computed;
  * `simulate`: generation.stop_state applied step after step to rows that keep their recorded finish — the state padt_stop_match must hold
    after every launch;
  * `criteria_from_stop_state` / `min_new_tokens_processor`: the hooked loop's twin of the three arguments — a stopping criterion written from
    stop_state and HF's own MinNewTokensLengthLogitsProcessor on host copies of the rows."""
from collections import namedtuple

import torch

from padt_amd.generation import NO_BUDGET, stop_state

CFG_EOS, EOS_LIST = 7, (9,)                 # the config's EOS id and the call's list
EOS_IDS = (CFG_EOS,) + EOS_LIST
PAD = 0
T_MAX = 12
LONG = list(range(11, 23))                  # 12 ids: as long as the token buffer
SEQS = [[3, 4], [4, 3, 4], [5], [5], LONG, [6, 7], [PAD], list(range(100, 132))]      # the last: 32 ids, the cap

Row = namedtuple("Row", "name tokens min_tokens max_tokens want preset")


def _row(name, head, min_tokens, max_tokens, want, preset=None):
    return Row(name, list(head) + [2] * (T_MAX - len(head)), min_tokens, max_tokens, want, preset)


# want = (finish_step, reason, index); preset = (finish_step, reason code, index): the row has a recorded finish on entry
ROWS = [
    _row("overlapping: [3,4] and [4,3,4] complete in one step → the lower index", [1, 4, 3, 4], 0, NO_BUDGET, (3, "stop", 0)),
    _row("a duplicated sequence → its first place; stop beats the budget of the same step", [6, 6, 5], 0, 3, (2, "stop", 2)),
    _row("the row holds the tail of a sequence longer than itself → no match; its budget ends it", LONG[6:], 0, 8, (7, "length", -1)),
    _row("a match completing below min_tokens is ignored and not matched later", [3, 4], 3, 6, (5, "length", -1)),
    _row("a match that starts below min_tokens and completes at it", [2, 3, 4], 3, NO_BUDGET, (2, "stop", 0)),
    _row("EOS, stop sequence [6,7] and budget in one step → eos", [1, 6, 7], 0, 3, (2, "eos", -1)),
    _row("finished on entry; its pad id is a stop sequence", [2, 9] + [PAD] * 10, 0, NO_BUDGET, (1, "eos", -1), preset=(1, 1, -1)),
    _row("twelve tokens equal to the twelve-id sequence: a match at the buffer's last step", LONG, 0, NO_BUDGET, (11, "stop", 4)),
]
REASON_CODE = {None: 0, "eos": 1, "stop": 2, "length": 3, "criteria": 4}


def initial_state():
    """(unfinished, finish_step, finish_reason, stop_index) lists as a generate starts them, the preset rows finished"""
    unf, step, reason, index = [], [], [], []
    for r in ROWS:
        p = r.preset
        unf.append(0 if p else 1), step.append(p[0] if p else -1), reason.append(p[1] if p else 0), index.append(p[2] if p else -1)
    return unf, step, reason, index


def simulate(n, state, rows=ROWS, seqs=SEQS, eos_ids=EOS_IDS):
    """one matcher launch at *step = n on `state` (lists, updated in place and returned): every row without a recorded finish is asked
    stop_state; nothing happens unless 1 <= n <= T_MAX"""
    unf, step, reason, index = state
    if 1 <= n <= T_MAX:
        for b, r in enumerate(rows):
            if reason[b] != 0:
                continue
            fin, why, i = stop_state(r.tokens, n, seqs, r.min_tokens, r.max_tokens, eos_ids)
            if fin:
                unf[b], step[b], reason[b], index[b] = 0, n - 1, REASON_CODE[why], i
    return state


# ------------------------------------------------------------------------------------------------------------ the hooked loop's twin
def criteria_from_stop_state(L, seqs, min_tokens, max_tokens, eos_ids):
    """A stopping criterion over (input_ids, scores): row b stops when stop_state says its last token ends it.  min_tokens / max_tokens: one
    value per row (max_tokens entries may be None).  EOS is the loop's own, so a row that stop_state ends by "eos" is left to it."""
    def crit(input_ids, scores):
        out = []
        for b, row in enumerate(input_ids[:, L:].tolist()):
            fin, why, _ = stop_state(row, len(row), seqs, min_tokens[b], max_tokens[b], eos_ids)
            out.append(bool(fin and why != "eos"))
        return torch.tensor(out, device=input_ids.device)
    return crit


def min_new_tokens_processor(L, min_tokens, eos_ids):
    """HF's MinNewTokensLengthLogitsProcessor per row (its class takes one minimum for the batch), on host copies of the rows"""
    from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor
    procs = [MinNewTokensLengthLogitsProcessor(L, int(m), [int(e) for e in eos_ids]) for m in min_tokens]

    def run(input_ids, scores):
        ids, rows = input_ids.cpu(), scores.to(torch.float32).cpu()
        out = torch.cat([p(ids[b: b + 1], rows[b: b + 1].clone()) for b, p in enumerate(procs)])
        return out.to(scores.device)
    return run
