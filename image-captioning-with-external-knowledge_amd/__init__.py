"""MI355X-native caption-decoder hot path of sonniki/image-captioning-with-external-knowledge.

Import as `ick_amd` (see /ick_amd.py).  Sub-modules:
  synth      seeded synthetic workloads (CPU tensors)
  build      hipcc recipe for csrc/ -> libick_amd.so (gfx950)
  lib        ctypes binding of the C ABI declared in include/ick_amd.h
  ops        per-op Python wrappers (device pointers from torch tensors)
  decoder    DecoderTransformer / Encoder engine shared by the three variants
  training   TrainStep: the fused cross-entropy training step
  bucket     ParamBucket: trained parameters, Adam moments and their average in flat fp32 tensors (pure torch)
  scst       SelfCriticalStep: self-critical sequence training on sampled captions (also `ick_amd.SelfCriticalStep`)
  cider      CiderD: CIDEr-D on token ids, on the device (also `ick_amd.CiderD`)
  metrics    CaptionMetrics: BLEU-1..4, ROUGE-L and pointer precision / recall on token ids, on the device, and
             MetricReward, their mix with CIDEr-D as an SCST reward (also `ick_amd.CaptionMetrics`)
  geo_metric GeoReferenceMetric: the geo variant's Jensen-Shannon geo-reference metric, counted on the device (also
             `ick_amd.GeoReferenceMetric`)
  geo_aware/models.py, knowledge_aware/models.py, news_knowledge_aware/models.py
             drop-in replacements for the reference's per-variant `models` module
"""
__version__ = "0.1.0"


def load_models(variant):
    """Return the drop-in `models` module of a variant ("geo" | "knowledge" | "news")."""
    import importlib
    name = {"geo": "geo_aware", "knowledge": "knowledge_aware", "news": "news_knowledge_aware"}[variant]
    return importlib.import_module("ick_amd.%s.models" % name)


def __getattr__(name):
    # lazy: importing the package must not load torch or the library
    if name == "SelfCriticalStep":
        from .scst import SelfCriticalStep
        return SelfCriticalStep
    if name == "CiderD":
        from .cider import CiderD
        return CiderD
    if name == "CaptionMetrics":
        from .metrics import CaptionMetrics
        return CaptionMetrics
    if name == "GeoReferenceMetric":
        from .geo_metric import GeoReferenceMetric
        return GeoReferenceMetric
    raise AttributeError("module 'ick_amd' has no attribute %r" % name)
