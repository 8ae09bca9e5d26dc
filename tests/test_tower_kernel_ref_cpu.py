"""No GPU: tests/tower_kernel_ref.py held to account.

  ledger      every __global__ kernel defined in csrc/vit.hip, text.hip and xlmr_text.hip is in the table or in the list of kernels
              tested elsewhere; the table reaches every form the launch functions pick (both patch gathers for both input types,
              the three LayerNorm kernels, NV 1 .. 8 of the row kernels); the planted token patterns all occur
  oracle      each restatement agrees with the oracle module that states it: the u8 normalisation and the gather with
              oracle/vit_ref.py, ln_pre's rows with vit_forward's first tap, the text tower's embedding and pooled row with a
              layers = 0 text_forward / siglip_text_forward, XLM-R's position ids, lens and mean pool with a layers = 0
              xlmr_text_forward (its tap and its output), BERT's absolute positions with clap_bert_ref.bert_hidden, the latent-query
              pool with siglip_ref._attention
  checker     the exact output passes every case; a NaN, a written guard row, an element never written and every planted fault
              fail, naming the case and the first bad row and column
  the 1 % cap bf16(ref32) differs from bf16(want64) in at most 1 % of the elements of every bf16 output: the inputs allow the
              condition the GPU test sets"""
import functools
import re
from pathlib import Path

import pytest
import torch

from oracle import clap_bert_ref, siglip_ref, text_ref, vit_ref, xlmr_text_ref
from tests import audio_kernel_ref as ak
from tests import tower_kernel_ref as tk

CSRC = Path(__file__).resolve().parent.parent / "wise_amd" / "csrc"
ALL = [(k, i) for k, cs in tk.CASES.items() for i in range(len(cs))]
F64 = torch.float64
TESTED_ELSEWHERE = {"attention_kernel", "cls_rows_kernel", "attn_oproj_fold_kernel"}      # tests/test_gpu_attention_exact.py


@functools.lru_cache(maxsize=None)
def problem(kernel, i):
    return tk.build(kernel, tk.CASES[kernel][i])


def find(kernel, **kw):
    for i, c in enumerate(tk.CASES[kernel]):
        if all(c[k] == v for k, v in kw.items()):
            return problem(kernel, i)
    raise KeyError((kernel, kw))


def fails(p, name, full, at=None):
    """the checker refuses `full` (a whole buffer, or the values a wrong kernel would have computed), naming the case"""
    o = p.outs[name]
    if full.shape[0] != o.rows + tk.GUARD:
        full = tk.as_output(o, full)
    assert tuple(full.shape) == (o.rows + tk.GUARD, o.cols) and full.dtype == o.dtype
    with pytest.raises(AssertionError, match=re.escape(p.what)) as e:
        tk.check(p, name, full)
    if at is not None:
        assert f"the first at row {at[0]}, column {at[1]}" in str(e.value), str(e.value)
    return True


# ------------------------------------------------------------------------------------------------ ledger
def test_every_kernel_of_the_three_files_is_accounted_for():
    defined = set()
    for name in ("vit.hip", "text.hip", "xlmr_text.hip"):
        defined |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", (CSRC / name).read_text()))
    tabled = {k for names in tk.KERNELS.values() for k in names}
    assert set(tk.KERNELS) == set(tk.CASES)
    assert tabled <= defined, tabled - defined
    assert not (tabled & TESTED_ELSEWHERE)
    assert defined == tabled | TESTED_ELSEWHERE, (defined - tabled - TESTED_ELSEWHERE, (tabled | TESTED_ELSEWHERE) - defined)


def test_the_table_reaches_every_form():
    assert {tk.patchify_form(c) for c in tk.CASES["patchify"]} == {f"{k}<{t}>" for k in ("patchify_kernel", "patchify8_kernel") for t in ("u8", "float")}
    off = [c for c in tk.CASES["patchify"] if c["off"]]
    assert off and all(tk.patchify_form(c).startswith("patchify_kernel<") and c["S"] == 32 and c["P"] == 16 for c in off)
    assert tk.kpad(14) == 640 and tk.kpad(8) == 192
    ln = {tk.layernorm_form(c["rows"], c["W"]) for c in tk.CASES["layernorm"]}
    assert ln >= {"layernorm_narrow_kernel", "layernorm_rows_kernel<1,4>", "layernorm_rows_kernel<2,4>", "layernorm_kernel<1>", "layernorm_kernel<16>"}
    nv = lambda W: (W // 4 + 63) // 64
    assert {nv(c["W"]) for c in tk.CASES["embed_lnpre"] if not c["fold"]} == {3, 4, 5, 7, 8}
    assert {nv(c["W"]) for c in tk.CASES["cls_ln"]} == {1, 2, 3, 5, 8}
    assert {nv(c["W"]) for c in tk.CASES["layernorm_dual"]} == {1, 3, 4, 16}
    # the issue's table, by count: nothing dropped
    assert {k: len(cs) for k, cs in tk.CASES.items()} == {"patchify": 12, "embed_pos": 6, "embed_lnpre": 6, "cls_ln": 90, "l2norm": 15,
                                                          "map_pool": 9, "hilo_rows": 4, "layernorm": 13, "layernorm_dual": 30,
                                                          "text_embed": 36, "xlmr_embed": 48, "xlmr_meanpool": 8}


def test_the_planted_token_patterns_all_occur():
    plants = {(c["pool"], pl) for i, c in enumerate(tk.CASES["text_embed"]) for pl in problem("text_embed", i).args["plants"]}
    assert plants >= {(0, "same lane"), (0, "adjacent"), (0, "last slot"), (0, "first slot"), (0, "only slot"),
                      (1, "partial"), (1, "all zero"), (1, "full")}
    for i, c in enumerate(tk.CASES["text_embed"]):
        p = problem("text_embed", i)
        ids = p.raw["ids"]
        if c["B"] * c["T"] >= 8:
            assert int(ids.max()) == tk.VOCAB - 1 and int(ids.min()) == 0, p.what
        for b, pl in enumerate(p.args["plants"]):
            if pl == "same lane":            # the first maximum and the second sit 64 apart: one lane of the kernel sees both
                at = (ids[b] == tk.VOCAB - 1).nonzero().reshape(-1).tolist()
                assert len(at) == 2 and at[1] - at[0] == 64
    for a in (0, 1):
        for pad in (0, 1):
            kinds = set()
            for i, c in enumerate(tk.CASES["xlmr_embed"]):
                if c["pos_abs"] == a and c["pad"] == pad:
                    p = problem("xlmr_embed", i)
                    kinds |= {("1", "2", "T-1", "T")[(1, 2, c["T"] - 1, c["T"]).index(n)] for n in p.args["lens"] if c["T"] >= 5}
                    assert int(p.raw["ids"].max()) == tk.VOCAB - 1 or c["T"] < 5 or max(p.args["lens"]) < 3, p.what
            assert kinds == {"1", "2", "T-1", "T"}, (a, pad, kinds)


# ------------------------------------------------------------------------------------------------ the restatements are the oracles'
def close(a, b, rtol=1e-5, atol=1e-5):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape
    assert torch.allclose(a, b, rtol=rtol, atol=atol), float((a - b).abs().max())


def test_u8_normalisation_and_gather_are_the_oracles():
    p = find("patchify", inp="u8", arch=0, S=28)
    img = p.raw["img"]
    assert torch.equal(tk.normalize_u8(img, 0), vit_ref.normalize_u8(img))
    for c in range(3):                       # every byte value in every channel
        assert len(set(img[:, c].reshape(-1).tolist())) == 256
    assert torch.equal(tk.normalize_u8(img, 1), (img.float() / 255.0 - 0.5) / 0.5)
    want = p.outs["patches"].want
    assert torch.equal(want[:, :588].reshape(2, 4, 588), vit_ref.patchify(vit_ref.normalize_u8(img), 14).to(torch.bfloat16))
    assert not bool(want[:, 588:].view(torch.int16).any()) and want.shape[1] == 640
    # float32 with two divisions is bf16(float64) but for a few ties of the rounding: the bit-for-bit expectation is the operation's
    x64 = p.raw["x64"]
    assert ak.flip_share(want, x64) < 0.002


def test_ln_pre_rows_are_the_oracles_first_tap():
    g = torch.Generator().manual_seed(3)
    B, S, P, W = 2, 16, 8, 128
    sd = {"visual.conv1.weight": torch.randn(W, 3, P, P, generator=g) * 0.05, "visual.class_embedding": torch.randn(W, generator=g),
          "visual.positional_embedding": torch.randn(5, W, generator=g), "visual.ln_pre.weight": 1 + 0.1 * torch.randn(W, generator=g),
          "visual.ln_pre.bias": 0.1 * torch.randn(W, generator=g), "visual.ln_post.weight": torch.ones(W), "visual.ln_post.bias": torch.zeros(W),
          "visual.proj": torch.eye(W)}
    img = torch.randn(B, 3, S, S, generator=g)
    taps = []
    vit_ref.vit_forward(sd, img, patch=P, heads=2, taps=taps)
    patch = (vit_ref.patchify(img, P) @ sd["visual.conv1.weight"].reshape(W, -1).t()).reshape(B * 4, W)
    n, _ = tk.embed_lnpre_ref(patch, sd["visual.class_embedding"], sd["visual.positional_embedding"], sd["visual.ln_pre.weight"],
                              sd["visual.ln_pre.bias"], B, 5)
    close(n, taps[0].reshape(B * 5, W))


@pytest.mark.parametrize("pool", [0, 2])
def test_text_embedding_and_pooled_row_are_the_oracles(pool):
    for T in (5, 77):
        p = find("text_embed", pool=pool, T=T, W=128)
        r, B = p.raw, p.case["B"]
        x, eot = p.outs["x"].want.reshape(B, T, 128), p.outs["eot"].want.reshape(-1).long()
        pooled = ak.layer_norm(x[torch.arange(B), eot], torch.ones(128), torch.zeros(128), 1e-5 if pool == 0 else 1e-6)
        if pool == 0:
            sd = {"token_embedding.weight": r["tok"], "positional_embedding": r["pos"], "ln_final.weight": torch.ones(128),
                  "ln_final.bias": torch.zeros(128), "text_projection": torch.eye(128)}
            out = text_ref.text_forward(sd, r["ids"], heads=2, normalize=False)
        else:
            sd = {"text.token_embedding.weight": r["tok"], "text.positional_embedding": r["pos"], "text.ln_final.weight": torch.ones(128),
                  "text.ln_final.bias": torch.zeros(128), "text.text_projection.weight": torch.eye(128),
                  "text.text_projection.bias": torch.zeros(128)}
            out = siglip_ref.siglip_text_forward(sd, r["ids"], heads=2, normalize=False)
        close(pooled, out)


def test_last_nonzero_pooling_is_msclaps_line():
    """sequence_lengths = ne(input_ids, 0).sum(-1) - 1, used as an index: -1 is the last position"""
    for i, c in enumerate(tk.CASES["text_embed"]):
        if c["pool"] == 1:
            p = problem("text_embed", i)
            ids = p.raw["ids"].long()
            seq = torch.ne(ids, 0).sum(-1) - 1
            x = torch.arange(c["T"]).expand(c["B"], c["T"])
            assert torch.equal(x[torch.arange(c["B"]), seq], p.outs["eot"].want.reshape(-1).long())


@pytest.mark.parametrize("pad", [1, 0])
def test_xlmr_embedding_lens_and_mean_pool_are_the_oracles(pad):
    for T in (5, 77):
        p = find("xlmr_embed", pos_abs=0, pad=pad, T=T, W=256)
        r, B, W = p.raw, p.case["B"], 256
        e = "text.transformer.embeddings."
        sd = {e + "word_embeddings.weight": r["word"], e + "position_embeddings.weight": r["pos"],
              e + "token_type_embeddings.weight": r["type0"].view(1, W), e + "LayerNorm.weight": torch.ones(W),
              e + "LayerNorm.bias": torch.zeros(W), "text.proj.0.weight": torch.eye(W), "text.proj.2.weight": torch.eye(W)}
        taps = []
        out = xlmr_text_ref.xlmr_text_forward(sd, r["ids"], heads=4, pad_id=pad, taps=taps, normalize=False)
        x = ak.layer_norm(p.outs["x"].want, torch.ones(W), torch.zeros(W)).reshape(B, T, W)
        close(x, taps[0])
        lens = p.outs["lens"].want.reshape(-1).tolist()
        assert lens == p.args["lens"]
        close(vit_ref.gelu(tk.meanpool_ref(x, lens)), out)


def test_bert_positions_are_the_oracles():
    p = find("xlmr_embed", pos_abs=1, pad=0, T=77, W=256)
    r, B, W = p.raw, p.case["B"], 256
    e = "base.embeddings."
    sd = {e + "word_embeddings.weight": r["word"], e + "position_embeddings.weight": r["pos"],
          e + "token_type_embeddings.weight": r["type0"].view(1, W), e + "LayerNorm.weight": torch.ones(W), e + "LayerNorm.bias": torch.zeros(W)}
    taps = []
    clap_bert_ref.bert_hidden(sd, r["ids"], heads=4, pad_id=0, taps=taps)
    close(ak.layer_norm(p.outs["x"].want, torch.ones(W), torch.zeros(W), clap_bert_ref.EPS).reshape(B, 77, W), taps[0], atol=1e-4)


def test_map_pool_is_the_oracles_attention():
    for data, T in (("random", 196), ("dominant", 65), ("equal", 729)):
        p = find("map_pool", data=data, T=T)
        kv, qv = p.raw["kv"].double().reshape(2, T, 256), p.raw["qv"].double()
        ref = siglip_ref._attention(qv.view(1, 1, 128).expand(2, 1, 128), kv[..., :128], kv[..., 128:], 2).reshape(2, 128)
        close(p.outs["o"].want, ref, rtol=1e-12, atol=1e-12)
        if data == "dominant":               # the weight of key T - 1 rounds to 1: the output is its value row
            assert torch.equal(p.outs["o"].want.float().to(torch.bfloat16), p.raw["kv"].reshape(2, T, 256)[:, T - 1, 128:])
        if data == "equal":
            close(p.outs["o"].want, kv[..., 128:].mean(dim=1), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("kernel,i", ALL, ids=[tk.case_id(k, tk.CASES[k][i]) for k, i in ALL])
def test_exact_outputs_pass_and_the_one_percent_condition_holds(kernel, i):
    p = problem(kernel, i)
    for name, o in p.outs.items():
        tk.check(p, name, tk.as_output(o))
        if o.kind == "bf16":
            flips = ak.flip_share(o.ref32.to(torch.bfloat16), o.want)
            assert flips <= 0.01, f"{p.what} {name}: bf16(ref32) != bf16(want64) in {100 * flips:.3f} % of the elements"
        live = torch.arange(o.rows) if o.keep is None else (~o.keep).nonzero().reshape(-1)
        r, col = int(live[len(live) // 2]), o.cols // 2
        # one element never written, one guard row written, (rows to leave alone) one of them written
        full = tk.as_output(o)
        full[r, col] = ak.nan_rows(1, 1, o.dtype)[0, 0]
        assert fails(p, name, full)
        full = tk.as_output(o)
        full[o.rows + 1, o.cols // 3] = 1
        assert fails(p, name, full)
        if o.keep is not None and bool(o.keep.any()):
            full = tk.as_output(o)
            full[int(o.keep.nonzero()[0]), 0] = 1
            assert fails(p, name, full)
        # ... and one wrong row out of all of them
        full = tk.as_output(o)
        last = int(live[-1])
        full[last] = (full[last].double() * 1.05 + 1).to(o.dtype)
        assert fails(p, name, full)


def test_position_id_off_by_one_fails():
    for i, c in enumerate(tk.CASES["xlmr_embed"]):
        p = problem("xlmr_embed", i)
        r, B, T = p.raw, c["B"], c["T"]
        pid = p.args["pid"] + (r["ids"].long() != c["pad"]).long() * (1 if not c["pos_abs"] else 0) + (1 if c["pos_abs"] else 0)
        x = ((r["word"][r["ids"].long()] + r["pos"][pid]) + r["type0"]).reshape(B * T, -1)
        assert fails(p, "x", x, at=(0, 0))
        assert fails(p, "lens", p.outs["lens"].want + 1, at=(0, 0))
    p = find("embed_pos", B=3, T=5)                      # pos[(row + 1) % T]
    x = (p.raw["patch"].reshape(3, 5, -1) + p.raw["pos"].roll(-1, 0)).reshape(15, -1)
    assert fails(p, "x", x, at=(0, 0))


def test_second_maximum_pooled_instead_of_the_first_fails():
    seen = set()
    for i, c in enumerate(tk.CASES["text_embed"]):
        p = problem("text_embed", i)
        if c["pool"] != 0:
            continue
        ids = p.raw["ids"].long()
        last = c["T"] - 1 - ids.flip(1).argmax(dim=-1)            # the LAST maximal index
        tie = (last != p.outs["eot"].want.reshape(-1)).nonzero().reshape(-1)
        if len(tie):
            assert fails(p, "eot", last.reshape(-1, 1), at=(int(tie[0]), 0))
            seen |= {p.args["plants"][int(b)] for b in tie}
    assert seen == {"same lane", "adjacent"}
    p = find("text_embed", pool=1, T=77)                          # the last non-zero index where the count belongs
    ids = p.raw["ids"].long()
    idx = 76 - (ids != 0).long().flip(1).argmax(dim=-1)
    assert fails(p, "eot", idx.reshape(-1, 1))


def test_mean_over_T_instead_of_lens_fails():
    for i, c in enumerate(tk.CASES["xlmr_meanpool"]):
        p = problem("xlmr_meanpool", i)
        x, lens = p.raw["x"].double(), p.raw["lens"].tolist()
        if not c["first"]:
            assert fails(p, "pooled", tk.meanpool_ref(x, lens, over_T=True), at=(0, 0))
            one_more = [min(c["T"], n + 1) for n in lens]         # a row past the length read: NaN
            assert fails(p, "pooled", tk.meanpool_ref(x, one_more), at=(0, 0))
        else:
            assert fails(p, "pooled", tk.meanpool_ref(x, [2, 2, 2, 2]))


def test_eps_dropped_fails():
    for kernel, name in (("cls_ln", "y"), ("layernorm", "y"), ("layernorm_dual", "xo"), ("layernorm_dual", "y")):
        hit = 0
        for i, c in enumerate(tk.CASES[kernel]):
            p = problem(kernel, i)
            r = p.raw
            if (kernel == "cls_ln" and c["B"] < 4) or c.get("eps", 1) < 1e-9:
                continue                                            # no constant row there (1e-12: eps is far below every variance)
            x = r["x"].double()[p.args["row"]] if kernel == "cls_ln" else r["x"].double()
            assert fails(p, name, ak.layer_norm(x, r["w"], r["b"], eps=0.0))
            hit += 1
        assert hit
    # ... and 1e-5 where 1e-6 belongs, on the row of tiny variance
    p = find("layernorm_dual", eps=1e-12, W=768, inplace=0)
    assert fails(p, "xo", ak.layer_norm(p.raw["x"].double(), p.raw["w"], p.raw["b"], eps=1e-6))
    p = find("embed_lnpre", fold=0, W=768)
    r = p.raw
    n, _ = tk.embed_lnpre_ref(r["patch"].double(), r["cls"].double(), r["pos"].double(), r["w"], r["b"], 3, 5, eps=1e-2)
    assert fails(p, "x", n)


def test_fold_form_faults():
    p = find("embed_lnpre", fold=1)
    r, o = p.raw, p.outs["hilo"]
    n, x = tk.embed_lnpre_ref(r["patch"].double(), r["cls"].double(), r["pos"].double(), r["w"], r["b"], 3, 5)
    assert torch.equal(n, o.want[:15])
    # rstd taken before the affine: that of the rows in front of the LayerNorm
    assert fails(p, "rstd", tk.row_rstd(x), at=(0, 0))
    # ... or of the normalised row without w and b: 1 / sqrt(1 + eps)
    assert fails(p, "rstd", tk.row_rstd(ak.layer_norm(x, torch.ones(768), torch.zeros(768))))
    # lo dropped, hi truncated instead of rounded, lo written where the gap is
    full = tk.as_output(o)
    full[-15 - tk.GUARD:-tk.GUARD] = 0
    assert fails(p, "hilo", full)
    full = tk.as_output(o)
    trunc = (n.float().view(torch.int32) & -65536).view(torch.float32)
    full[:15], full[-15 - tk.GUARD:-tk.GUARD] = trunc.to(torch.bfloat16), (n - trunc.double()).float().to(torch.bfloat16)
    assert fails(p, "hilo", full)
    full = tk.as_output(o)
    full[15:30] = full[-15 - tk.GUARD:-tk.GUARD]
    assert fails(p, "hilo", full, at=(0, 0))
    # the class row taken for every row / patch rows one off
    p = find("embed_lnpre", fold=0, W=1664)
    r = p.raw
    n, _ = tk.embed_lnpre_ref(r["patch"].roll(1, 0).double(), r["cls"].double(), r["pos"].double(), r["w"], r["b"], 3, 5)
    assert fails(p, "x", n, at=(1, 0))


def test_reciprocal_multiply_in_the_u8_normalisation_fails():
    """x * (1 / 255) moves a third of the 768 (byte, channel) values by one fp32 step.  With mean = std = 0.5 three of them cross a bf16
    rounding boundary (one byte value per channel): every arch 1 case fails.  With CLIP's constants none of the 768 does: that
    form returns the same bf16 bits for every possible input, so no output can tell it from the division (asserted, not assumed)"""
    for i, c in enumerate(tk.CASES["patchify"]):
        if c["inp"] == "u8":
            p = problem("patchify", i)
            wrong = tk.patch_rows(tk.normalize_u8(p.raw["img"], c["arch"], reciprocal=True), c["P"]).to(torch.bfloat16)
            if c["arch"] == 1:
                assert fails(p, "patches", wrong)
            else:
                assert torch.equal(wrong, p.outs["patches"].want)
    p = find("patchify", inp="u8", arch=0, S=16)                  # the wrong set of constants; a truncating bf16 conversion
    assert fails(p, "patches", tk.patch_rows(tk.normalize_u8(p.raw["img"], 1), 8).to(torch.bfloat16))
    x = tk.patch_rows(tk.normalize_u8(p.raw["img"], 0), 8)
    assert fails(p, "patches", (x.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16))
    p = find("patchify", inp="f32", S=28)                         # py and px swapped in the gather; a padding column written
    assert fails(p, "patches", tk.patch_rows(p.raw["img"].transpose(2, 3), 14).reshape(2, 2, 2, 640).transpose(1, 2).reshape(8, 640).to(torch.bfloat16))
    full = tk.as_output(p.outs["patches"])
    full[3, 588] = 1
    assert fails(p, "patches", full, at=(3, 588))


def test_last_token_slice_left_out_of_the_pool_fails():
    for i, c in enumerate(tk.CASES["map_pool"]):
        if c["T"] > 64:
            p = problem("map_pool", i)
            assert fails(p, "o", tk.map_pool_ref(p.raw["kv"].double(), p.raw["qv"], 2, c["T"], 128, skip_last_slice=True))
    p = find("map_pool", data="random", T=196)                    # heads swapped; scale 1 / 64 where 1 / 8 belongs
    want = p.outs["o"].want
    assert fails(p, "o", torch.cat([want[:, 64:], want[:, :64]], dim=1), at=(0, 0))
    assert fails(p, "o", tk.map_pool_ref(p.raw["kv"].double(), p.raw["qv"] / 8, 2, 196, 128))


def test_other_row_faults_fail():
    p = find("cls_ln", pos=1, B=5, T=77, W=768)                   # row 0 pooled where pos[b] belongs
    r = p.raw
    assert fails(p, "y", ak.layer_norm(r["x"].double()[torch.arange(5) * 77], r["w"], r["b"]), at=(1, 0))
    p = find("l2norm", rows=7, D=100)                             # an epsilon the reference does not have; the sum over 64 of 100
    e = p.raw["e"].double()
    assert fails(p, "out", e / (e.norm(dim=-1, keepdim=True) + 1e-6), at=(0, 0))
    assert fails(p, "out", e / e[:, :64].norm(dim=-1, keepdim=True))
    p = find("hilo_rows", stride=5)                               # lo dropped; stride ignored
    hi = p.raw["hi"][:11 * 768].reshape(11, 768).float()
    want = p.outs["out"].want
    assert fails(p, "out", hi[::5])
    assert fails(p, "out", torch.cat([want[:1], want[:2]]), at=(1, 0))
    p = find("text_embed", pool=0, T=77, W=384)                   # the position row of t + 1
    r = p.raw
    x = (r["tok"][r["ids"].long()] + r["pos"].roll(-1, 0)).reshape(3 * 77, 384)
    assert fails(p, "x", x, at=(0, 0))
