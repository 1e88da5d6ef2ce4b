"""Greedy caption generation over a test split, mirroring evaluate() of the reference's eval.py
(geo-aware/eval.py:46-125; knowledge-aware/eval.py:46-200 for the fact tokens): encoder -> decoder.predict ->
token ids -> text (vocabulary words, entity names and fact objects decoded from their integer encodings) ->
generated_captions.csv.  With metrics= / refs= the written rows are also scored on the device (metrics.CaptionMetrics:
BLEU-1..4, ROUGE-L, pointer precision / recall on token ids -- the reference's compute_eval_metrics.py without METEOR
and spaCy's entities).  With geo_metric= the geo variant's Jensen-Shannon geo-reference metric (its
jensen_shannon_metric.py, eval.py:116,125) is counted on the device as well (geo_metric.GeoReferenceMetric).  The other
domain metrics of the reference (fact accuracy...) are CPU text statistics outside this path."""
import os

import numpy as np
import pandas as pd
import torch

from . import utils as ut


def detokenize(seq, word_map, rev_word_map, entity_names, fact_names=None):
    """seq: iterable of token ids of ONE caption; entity_names (K, 2+50) / fact_names (F, 2+50) integer-encoded
    names [idx, length, chars...] as produced by the reference's preprocessing."""
    V = len(word_map)
    K = entity_names.shape[0]
    special = {word_map["<start>"], word_map["<end>"], word_map["<pad>"]}
    words = []
    for tok in seq:
        tok = int(tok)
        if tok < V:
            if tok not in special:
                words.append(rev_word_map[tok])
        elif tok < V + K or fact_names is None:
            k = tok - V
            words.append("<unk_ent>" if k >= K else ut.int_to_str(entity_names[k][2:].tolist(), int(entity_names[k][1])))
        else:
            j = tok - V - K
            words.append("<unk_fact>" if j >= fact_names.shape[0]
                         else ut.int_to_str(fact_names[j][2:].tolist(), int(fact_names[j][1])))
    text = " ".join(words)
    if not text.endswith(".") and text.count(".") > 1:       # drop a trailing unfinished sentence
        text = ".".join(text.split(".")[:-1]) + "."
    return text


@torch.no_grad()
def evaluate(encoder, decoder, loader, word_map, max_caption_len=30, out_csv="generated_captions.csv", device="cuda",
             sample=None, attention_out=None, beam=None, metrics=None, refs=None, geo_metric=None):
    """sample=None: greedy decode (predict), one CSV row per image.  sample = a dict of predict_sample keyword arguments
    (num_samples, temperature, top_k, top_p, seed, and the decoding rules no_repeat_ngram_size, min_len): sampled
    decode, one CSV row per (image, sample) with the columns image (running index over the loader), sample,
    generated_caption; an explicit seed is advanced by one per batch.  beam = a dict of predict_beam keyword arguments
    (beam_size, length_penalty, no_repeat_ngram_size, min_len, num_beam_groups, diversity_penalty, return_groups):
    beam-search decode, one CSV row per image (the best hypothesis); with return_groups (diverse beam search), one CSV
    row per (image, group) with the columns image, group, generated_caption, the best hypothesis of each group;
    force_tokens (constrained beam search) is a callable fn(batch_index, batch) -> the (B, C) forced column ids of
    that batch, since one tensor cannot fit every batch; column_bias (in beam or sample) is predict_beam's value -- a
    dict or a pair for every batch -- or such a callable, and prefix (in beam or sample) is predict_beam's value or such a
    callable; beam and sample together are a ValueError.
    attention_out: a path for one .npz of the decoder's cross-attention (return_attention of predict / predict_sample):
    "attention" float16 (N, max_len, S), the last decoder layer's weights averaged over its heads, one row per CSV row;
    "tokens" int64 (N, max_len); "P", "K", "F": how the S memory rows split into image, entity and fact rows.  With
    beam, the weights are those of the best hypothesis (of each group with return_groups).
    metrics: a metrics.CaptionMetrics, with refs = fn(batch_index, batch) -> the (B, M, Lr) (or (B, L)) int64 reference
    captions of that batch: every written row is scored on the device against its image's references (sampled rows and
    group rows through image_index), the batches' totals are added on the device and read once at the end.  Returns
    (captions, sequences, result) with result = CaptionMetrics.result()'s dict, and writes
    metric_scores_for_generated_captions.csv next to out_csv: the CSV's own columns plus Bleu_1..Bleu_4, ROUGE_L
    (sentence scores), pointer_hits, pointer_generated, pointer_reference.
    geo_metric: a geo_metric.GeoReferenceMetric: every written row's geo references are counted on the device against
    its image's entity features and names (batch[4], batch[5]; sampled rows and group rows through image_index, row_offset
    = the number of rows written before the batch), the batches' histograms are added on the device and read once at the
    end; result gains "geo_js" = GeoReferenceMetric.result()'s dict.  Returns (captions, sequences, result) when either
    metrics or geo_metric is given; without them: (captions, sequences) as before."""
    if beam is not None and sample is not None:
        raise ValueError("evaluate: beam and sample are two different decoders; pass one of them")
    if (metrics is None) != (refs is None) or (refs is not None and not callable(refs)):
        raise ValueError("evaluate: metrics= (a CaptionMetrics) and refs= (fn(batch_index, batch) -> references) go together")
    decoder.eval()
    encoder.eval()
    rev = {v: k for k, v in word_map.items()}
    captions, sequences, rows = [], [], []
    n = int(sample.get("num_samples", 1)) if sample is not None else 1
    groups = beam is not None and bool(beam.get("return_groups", False))
    if groups:
        n = int(beam.get("num_beam_groups", 1))         # predict_beam's column b*G + g: image b, group g
    # precomputed feature maps go to predict() as they are: Encoder.conv1 then runs inside the captured decode graph
    # beside the context encoders (decoder.attach_encoder); raw images go through the encoder's trunk first
    decoder.attach_encoder(encoder)
    img_buf = None
    attn_rows, attn_split = [], None
    want_attn = attention_out is not None
    totals, metric_rows = None, []
    geo_counts = None
    for bi, batch in enumerate(loader):                       # any batch size: captions decode independently
        ent, names = batch[4], batch[5]
        has_facts = len(batch) > 6
        extra = (batch[6].to(device),) if has_facts else ()
        feature_map = batch[0].dim() == 4 and batch[0].shape[1] == encoder.encoder_dim
        if feature_map and img_buf is not None and img_buf.shape == batch[0].shape:
            # the host-to-device copy lands straight in the decode graph's own input buffer (widening a float16 feature
            # file on the way): predict() then skips its device-to-device copy of the feature map (51 MB at batch 32)
            img_buf.copy_(batch[0], non_blocking=True)
            image = img_buf
        else:
            image = batch[0].to(device)
        enc_in = image if feature_map else encoder(image)
        attn = None
        if beam is not None:
            kw = dict(beam)
            kw.pop("return_all", None)
            if kw.get("force_tokens") is not None:           # a callable: the forced columns of this batch
                kw["force_tokens"] = kw["force_tokens"](bi, batch)
            if callable(kw.get("column_bias")):              # the bias of this batch
                kw["column_bias"] = kw["column_bias"](bi, batch)
            if callable(kw.get("prefix")):                   # the caption prefixes of this batch
                kw["prefix"] = kw["prefix"](bi, batch)
            seq = decoder.predict_beam(enc_in, max_caption_len, ent, *extra, return_attention=want_attn, **kw)
        elif sample is None:
            seq = decoder.predict(enc_in, max_caption_len, ent, *extra, return_attention=want_attn)  # (max_len, B)
        else:
            kw = dict(sample)
            if kw.get("seed") is not None:       # a batch's caption b would otherwise reuse the noise of every other batch's b
                kw["seed"] = int(kw["seed"]) + bi
            kw.pop("return_log_probs", None)
            if callable(kw.get("column_bias")):
                kw["column_bias"] = kw["column_bias"](bi, batch)
            if callable(kw.get("prefix")):
                kw["prefix"] = kw["prefix"](bi, batch)
            seq = decoder.predict_sample(enc_in, max_caption_len, ent, *extra, return_attention=want_attn, **kw)
        if want_attn:
            seq, attn = seq
            # (max_len, rows, layers, H, S) -> last layer, mean over heads -> (rows, max_len, S)
            attn_rows.append(attn[:, :, -1].mean(dim=2).transpose(0, 1).to(torch.float16).cpu())
            K, F = ent.shape[1], (batch[6].shape[1] if has_facts else 0)
            split = (attn.shape[-1] - K - F, K, F)
            if attn_split is not None and attn_split != split:
                raise ValueError("evaluate(attention_out=...): batches with different memory sizes %s / %s"
                                 % (attn_split, split))
            attn_split = split
        if metrics is not None:
            # rows b of seq: image b // n of this batch; everything stays on the device until the loop ends
            cand = seq.t().contiguous()
            idx = torch.arange(cand.shape[0], device=cand.device, dtype=torch.int32) // n
            mr = metrics(cand, idx, refs(bi, batch))
            t = metrics.totals(mr)
            totals = t if totals is None else totals + t
            metric_rows.append(mr)
        if geo_metric is not None:
            cand = seq.t().contiguous()
            idx = torch.arange(cand.shape[0], device=cand.device, dtype=torch.int32) // n
            gc = geo_metric(cand, idx, ent, names, row_offset=len(sequences))
            geo_counts = gc if geo_counts is None else geo_counts + gc
        bufs = decoder.input_buffers() if feature_map else None
        img_buf = bufs[0] if bufs is not None and bufs[0] is not None and bufs[0].dim() == 4 else None
        for b in range(seq.shape[1]):
            ids = seq[:, b].tolist()
            sequences.append(ids)
            k = b // n
            captions.append(detokenize(ids, word_map, rev, names[k], batch[7][k] if has_facts else None))
            rows.append((len(rows) // n, b % n))
    if want_attn:
        P, K, F = attn_split if attn_split is not None else (0, 0, 0)
        np.savez(attention_out, attention=torch.cat(attn_rows).numpy() if attn_rows else np.zeros((0, max_caption_len, 0),
                 np.float16), tokens=np.asarray(sequences, dtype=np.int64).reshape(-1, max_caption_len), P=P, K=K, F=F)
    if groups:
        columns = {"image": [r[0] for r in rows], "group": [r[1] for r in rows], "generated_caption": captions}
    elif sample is None:
        columns = {"generated_caption": captions}
    else:
        columns = {"image": [r[0] for r in rows], "sample": [r[1] for r in rows], "generated_caption": captions}
    if out_csv:
        pd.DataFrame(columns).to_csv(out_csv, index=False)
    if metrics is None and geo_metric is None:
        return captions, sequences
    result = metrics.result(totals) if totals is not None else {}
    if geo_metric is not None:
        result["geo_js"] = geo_metric.result(geo_counts) if geo_counts is not None else None
    if metrics is not None and out_csv and metric_rows:
        bleu = torch.cat([m.bleu for m in metric_rows]).cpu().numpy()
        ptr = torch.cat([m.pointers for m in metric_rows]).cpu().numpy()
        for k in range(4):
            columns["Bleu_%d" % (k + 1)] = bleu[:, k]
        columns["ROUGE_L"] = torch.cat([m.rouge_l for m in metric_rows]).cpu().numpy()
        for k, name in enumerate(("pointer_hits", "pointer_generated", "pointer_reference")):
            columns[name] = ptr[:, k]
        pd.DataFrame(columns).to_csv(os.path.join(os.path.dirname(out_csv), "metric_scores_for_generated_captions.csv"),
                                     index=False)
    return captions, sequences, result
