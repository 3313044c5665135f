"""Generate tests/golden/aux_outputs.npz: slots 6, 7 and 9 of the REFERENCE's 10-tuple as index maps into the aux rows.

Run by hand in the build container only:   python tests/golden/make_golden_aux.py
The reference is imported through make_golden (its config, model builder and synthetic video; that module only writes
fixtures under its __main__ guard) and run by a runner of its own; no existing fixture is rewritten.

prepare_inputs_labels_for_multimodal returns, for mm_projector_type == "sva" (tdc/cambrian_arch.py:1187-1193, 1295-1303,
1833-1844), vision_tower_aux_feature_list_final (out[6]), vision_tower_aux_attention_masks_list_final (out[7]) and
global_context_feature_final (out[9]).  Every row of out[6][i] is, bit for bit, one row of the hooked mm_projector_aux_i
output, which pipeline_*.npz already holds as out_aux{i}; every row of out[9] is one frame's mean row.  So a case stores
  feat_src{0,1}  int32 [n, r*r]  row of out_aux{i}.reshape(T*P, C) behind every element of out[6][i] (exactly one match each)
  mask{0,1}      bool  [n, r*r]  out[7][i]
  ctx_src        int32 [n]       frame behind every row of out[9]
  ctx_rows       fp32  [T, C]    the frames' mean rows (out[9] == ctx_rows[ctx_src])
  final_size     int   [T, 2]    out[8]
under the key "<case>::<name>".  Cases: (a) pipeline_T40, (b) pipeline_T10_land, (c) the inputs and weights of (b) with
image_size (480, 640) - the one whose masks are not all True (its aux rows are (b)'s: the image size does not enter before the
rearrangement).

Fixtures written:
  aux_outputs.npz       the three cases
  manifest_aux.json     shapes, window counts, versions
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import synth  # noqa: E402

# name -> (pipeline fixture that holds the inputs, weights and out_aux{0,1}; T; seed; image_size; prompt; compare out[4])
CASES = {
    "T40": ("pipeline_T40.npz", 40, 0, (384, 384), "what happens in the video ?", True),
    "T10_land": ("pipeline_T10_land.npz", 10, 1, (360, 640), "describe the clip", True),
    "T10_480x640": ("pipeline_T10_land.npz", 10, 1, (480, 640), "describe the clip", False),
}


def run_reference(T, seed, image_size, prompt, px=126):
    """make_golden.run_pipeline's model and inputs (same seeds), the reference's prepare_inputs_labels_for_multimodal, the
    hooked mm_projector_aux_i outputs -> (out, aux0, aux1)"""
    cfg = mg.make_config()
    lm = mg.build_lm(cfg, seed)
    basis, coef = synth.make_basis_and_coef(T, px, seed=1234 + seed)
    vid = torch.from_numpy(synth.video_from_basis(basis, coef))
    images = [vid.unsqueeze(0), (vid + 0.01).unsqueeze(0)]
    ids = torch.tensor([[1001, 1002, 1003, -200, 1004, 1005, 1006, 1007, 1008]], dtype=torch.long)
    cap, hooks = {}, []
    for i in range(2):
        mod = getattr(lm.model, "mm_projector_aux_%d" % i)
        hooks.append(mod.register_forward_hook(lambda m, inp, out, i=i: cap.setdefault(i, []).append(out.detach().clone())))
    with torch.inference_mode():
        out = lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images, image_sizes=[image_size],
                                                      video_indices=[None], prompts=[prompt], audios=[None])
    for h in hooks:
        h.remove()
    assert len(cap[0]) == 1 and len(cap[1]) == 1
    return out, cap[0][0].numpy(), cap[1][0].numpy()


def row_sources(rows, table):
    """for every row of `rows` the index of the ONE row of `table` with the same bytes"""
    where = {}
    for j, r in enumerate(np.ascontiguousarray(table)):
        where.setdefault(r.tobytes(), []).append(j)
    src = np.zeros(rows.shape[0], dtype=np.int32)
    for i, r in enumerate(np.ascontiguousarray(rows)):
        hit = where.get(r.tobytes(), [])
        assert len(hit) == 1, "row %d has %d matches" % (i, len(hit))
        src[i] = hit[0]
    return src


def make_case(name, fixture, T, seed, image_size, prompt, same_embeds):
    z = np.load(os.path.join(HERE, fixture))
    out, aux0, aux1 = run_reference(T, seed, image_size, prompt)
    if same_embeds:
        assert np.array_equal(out[4].numpy(), z["out_inputs_embeds"]), "%s: inputs_embeds differ from %s" % (name, fixture)
    assert np.array_equal(aux0, z["out_aux0"]) and np.array_equal(aux1, z["out_aux1"]), "%s: aux rows differ" % name
    C = aux0.shape[-1]
    arrs = {}
    final_size = np.asarray(out[8], dtype=np.int64).reshape(-1, 2)
    n = int((final_size[:, 0] * final_size[:, 1]).sum())
    for i, a in enumerate((aux0, aux1)):
        feat, mask = out[6][i].numpy(), out[7][i].numpy()
        assert feat.shape[0] == n and feat.shape[2] == C and mask.shape == feat.shape[:2] and mask.dtype == np.bool_
        table = a.reshape(-1, C)
        src = row_sources(feat.reshape(-1, C), table).reshape(feat.shape[:2])
        assert np.array_equal(table[src], feat)
        arrs["feat_src%d" % i], arrs["mask%d" % i] = src, mask
    ctx = out[9].numpy()
    assert ctx.shape == (n, 1, C)
    ctx_src = np.repeat(np.arange(final_size.shape[0], dtype=np.int32), final_size[:, 0] * final_size[:, 1])
    first = np.concatenate([[0], np.cumsum(final_size[:, 0] * final_size[:, 1])[:-1]])
    ctx_rows = ctx[first, 0].astype(np.float32)
    assert np.array_equal(ctx_rows[ctx_src], ctx[:, 0])
    arrs.update(ctx_src=ctx_src, ctx_rows=ctx_rows, final_size=final_size, image_size=np.asarray(image_size))
    masked = int((~arrs["mask0"].all(-1)).sum())
    return arrs, dict(fixture=fixture, T=T, seed=seed, image_size=list(image_size), n=n, rr=int(arrs["mask0"].shape[1]), C=int(C),
                      final_size=[int(v) for v in final_size[0]], windows_with_masked_entries=masked)


if __name__ == "__main__":
    import transformers
    man = dict(torch=torch.__version__, transformers=transformers.__version__, cases={})
    arrs = {}
    for name, case in CASES.items():
        a, man["cases"][name] = make_case(name, *case)
        arrs.update({"%s::%s" % (name, k): v for k, v in a.items()})
    path = os.path.join(HERE, "aux_outputs.npz")
    np.savez_compressed(path, **arrs)
    with open(os.path.join(HERE, "manifest_aux.json"), "w") as f:
        json.dump(man, f, indent=1)
    print("wrote aux_outputs.npz %.1f KB" % (os.path.getsize(path) / 1024))
    print(json.dumps(man, indent=1))
