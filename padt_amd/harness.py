"""Dataset loop of the reference's evaluation (eval/evaluation_scripts/utils.py:176-266, `infer_dataset`) on the MI355X path:
rank-strided batches (utils.py:181-182), generate → parse → vl_decode through the throughput runner, the caller-side
post-processing (utils.py:252-266) and the two JSONL files with the reference's names and record schema:

    {datasetname}_{rank}_pred_comp_{suffix}.json      {"image_id", "completion"}                      one line per sample
    {datasetname}_{rank}_pred_results_{suffix}.json   {"image_id", "score", "category", "bbox", "mask"} one line per object

Tokenisation / chat templating is the caller's (`prepare`): it needs the checkpoint's tokenizer files, which are not part of
this repository.  `prepare(samples) -> dict(input_ids (local VRT ids), attention_mask, pixel_values, image_grid_thw,
image_sizes [(w, h)], ids [image_id])`; optionally `image_index` (several samples on one image: generate(image_index=), with
`pixel_values` / `image_grid_thw` holding each image once), `prefix` (a handle of model.encode_prefix the batch's rows continue:
generate(prefix=), with `pixel_values` / `image_grid_thw` left out or `None`), `forced_tokens` (the batch's completion tokens to force:
generate(forced_tokens=)), `patch_bias` (one entry per sample over its own patches: generate(patch_bias=)), `min_tokens` / `max_tokens`
(one int per sample: generate(min_tokens=, max_tokens=)) and `frequency_penalty` / `presence_penalty` / `patch_suppression` (one entry per
sample: generate()'s count edits).
"""
import json
import os
from typing import Callable, Sequence

from .pipeline import PipelinedRunner, rank_batches
from .postprocess import postprocess_results


def infer_dataset(model, processor, dataset: Sequence, prepare: Callable, output_dir: str, batch_size: int = 1,
                  datasetname: str = "coco", suffix: str = "", rank: int = 0, world: int = 1, max_new_tokens: int = 1024,
                  depth: int = 2, merge: int = 4, schedule=None, repetition_penalty=None, eos_token_id=None,
                  token_automaton=None, logit_bias=None, exponential_decay_length_penalty=None, stop_sequences=None, min_tokens=None,
                  max_tokens=None, frequency_penalty=None, presence_penalty=None, patch_suppression=None, beam_width=None, n_best=None,
                  beam_length_penalty=None, beam_early_stopping=None):
    """repetition_penalty / eos_token_id: None = the checkpoint's generation_config.json (model.generation_config), as HF's
    generate() inside the reference's loop applies it (utils.py:230-236 → padt.py:436).
    token_automaton: generate(token_automaton=) for every batch of the run (e.g. the dataset's category names followed by their VRTs).
    logit_bias / exponential_decay_length_penalty: generate()'s, for every batch of the run; a batch's own patch prior comes from `prepare`.
    stop_sequences / min_tokens / max_tokens: generate()'s, for every batch of the run (one value each; `prepare` may return per-row
    `min_tokens` / `max_tokens` lists of its batch, which win).
    frequency_penalty / presence_penalty / patch_suppression: generate()'s count edits, for every batch of the run (one value each; `prepare`
    may return per-row lists of its batch under the same names, which win).
    beam_width / n_best / beam_length_penalty / beam_early_stopping: generate()'s beam search, for every batch of the run; every sample then
    writes n_best completions and result sets under its image id, best first."""
    os.makedirs(output_dir, exist_ok=True)
    f_res = os.path.join(output_dir, f"{datasetname}_{rank}_pred_results_{suffix}.json")
    f_comp = os.path.join(output_dir, f"{datasetname}_{rank}_pred_comp_{suffix}.json")
    for f in (f_res, f_comp):
        open(f, "w").close()                                      # utils.py:184-188: truncate
    runner = PipelinedRunner(model, processor, depth=depth, merge=merge)
    meta = []                                                     # per submitted batch, in submission (= completion) order

    def drain(finished):
        for decoded, completions, labels, vrts in finished:
            m = meta.pop(0)
            with open(f_comp, "a") as fc:
                for i, completion in enumerate(completions):
                    fc.write(json.dumps({"image_id": m["ids"][i],
                                         "completion": completion.replace("<|endoftext|>", "").replace("<|im_end|>", "")}) + "\n")
            if decoded["pred_boxes"].shape[0] == 0:               # utils.py:253-254
                continue
            with open(f_res, "a") as fr:
                for r in postprocess_results(decoded, labels, m["image_sizes"]):
                    fr.write(json.dumps({"image_id": m["ids"][r["sample_idx"]], "score": r["score"], "category": r["category"],
                                         "bbox": list(r["bbox"]), "mask": r.get("rle")}) + "\n")

    n = 0
    for idx in rank_batches(len(dataset), batch_size, rank, world):
        if idx >= len(dataset):                                   # utils.py:196: ranks past the end skip the work
            continue
        b = prepare(dataset[idx: idx + batch_size])
        rep = (n_best or 1) if beam_width is not None else 1      # a beam batch returns n_best rows per sample
        meta.append({"ids": [i for i in b["ids"] for _ in range(rep)], "image_sizes": [z for z in b["image_sizes"] for _ in range(rep)]})
        extra = {"image_index": b["image_index"]} if b.get("image_index") is not None else {}
        if b.get("prefix") is not None:
            extra["prefix"] = b["prefix"]
        extra["forced_tokens"] = b.get("forced_tokens")           # None: nothing forced
        extra["patch_bias"] = b.get("patch_bias")                 # None: no prior over the patches
        extra["min_tokens"] = b.get("min_tokens", min_tokens)     # the batch's own rows, else the run's value
        extra["max_tokens"] = b.get("max_tokens", max_tokens)
        extra["frequency_penalty"] = b.get("frequency_penalty", frequency_penalty)
        extra["presence_penalty"] = b.get("presence_penalty", presence_penalty)
        extra["patch_suppression"] = b.get("patch_suppression", patch_suppression)
        drain(runner.submit(b["input_ids"], b["attention_mask"], b.get("pixel_values"), b.get("image_grid_thw"),
                            max_new_tokens=max_new_tokens, schedule=schedule, repetition_penalty=repetition_penalty,
                            eos_token_id=eos_token_id, token_automaton=token_automaton, logit_bias=logit_bias,
                            exponential_decay_length_penalty=exponential_decay_length_penalty, stop_sequences=stop_sequences,
                            beam_width=beam_width, n_best=n_best, beam_length_penalty=beam_length_penalty,
                            beam_early_stopping=beam_early_stopping, **extra))
        n += len(b["ids"])
    drain(runner.flush())
    return {"samples": n, "results_file": f_res, "completions_file": f_comp}
