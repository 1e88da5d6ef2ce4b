"""The geo variant's Jensen-Shannon geo-reference metric on the device: does a caption use its geographic context the
way the training captions do?  (The reference's JSGeoMetric, geo-aware/jensen_shannon_metric.py, run from its eval.py.)

Whenever a caption puts an entity pointer behind a spatial preposition, the entity's distance bin, azimuth bin and OSM
type are recorded; at the end, per preposition, the Jensen-Shannon distance between those histograms and the train
set's is reported, beside the same for a random entity of the image.  The definition, on token ids, is the contract
(include/ick_amd.h states the same):

* Terms, in this order: near, along, across, in, north, south, east, west.  A term's trigger is its word's id; the
  azimuth words are north_of, south_of, east_of, west_of if the word map has north_of, else north, south, east, west.
  Words the map lacks never trigger.  V = len(word_map).
* Position i >= 1 of a caption row with token t >= V counts when the previous token p0 < V and one of these holds:
  p0 is a trigger;  i >= 2, p1 is a trigger and p0 is one of {of, the, a};  i >= 3, p2 is a trigger, p1 == of and p0 is
  one of {the, a} -- the term is the trigger that matched -- and k = t - V < K, and the effective name of entity k does
  not contain "unk_ent".  The whole row is scanned (after <end> there is only <pad>).
* The effective name of an entity is the first min(length, 50) characters of its integer-encoded name [idx, length,
  chars...]; a negative length gives all 50 (utils.int_to_str).
* A counted reference adds 1 to its term's n_occurrences; terms near, along, across, in: 1 to the first distance bin
  with lo <= x < hi (float64 edges; nothing if there is none); north..west: the same for the azimuth; along, across, in:
  1 to type x when x is an exact integer in [0, n_types).  Entity features: column 1 distance, 2 azimuth, 4 type.
* Random-entity baseline: the same increments for entity s[j], s = the image's non-unk_ent entity slots in slot order,
  j = x mod len(s), x = the first word of Philox-4x32-10 of counter (i, row_offset + n, 0, 0) under the key (seed's low,
  high 32 bits), n = the row's index in the call.  (The reference draws with Python's random.choice.)
* Result: prob = count / n_occurrences per bin; the JS distance sqrt(0.5 KL(p || m) + 0.5 KL(q || m)), m = (p + q) / 2,
  log base 2, zero entries skipped, against the train distribution's *_probs; float64 on the host.

The kernel (csrc/geo_metric.hip, ick_geo_reference_counts) adds the histograms up with integer atomics, so the counts
are the same bits on every run; result() reads them once.
"""
import collections
import math
import os
import pickle

import torch

from . import ops
from .lib import IckError

TERMS = ("near", "along", "across", "in", "north", "south", "east", "west")
FEATURES = {"near": ("distance",), "along": ("distance", "type"), "across": ("distance", "type"),
            "in": ("distance", "type"), "north": ("azimuth",), "south": ("azimuth",), "east": ("azimuth",),
            "west": ("azimuth",)}
_COL0 = {"distance": 1, "azimuth": 1 + ops.GEO_MAX_BINS, "type": 1 + 2 * ops.GEO_MAX_BINS}


class GeoReferenceCounts(collections.namedtuple("GeoReferenceCounts", "generated random marks")):
    """Device tensors of one call: generated, random (8, 1 + 64 + 64 + n_types padded to 64) int32 histograms -- row =
    term, column 0 n_occurrences, then 64 distance bins, 64 azimuth bins and the types; marks (N, T) int32: -1 where no
    reference is counted, else term << 24 | random entity << 12 | entity.  a + b adds two batches' histograms on the
    device (the sum carries no marks)."""
    __slots__ = ()

    def __add__(self, other):
        if not isinstance(other, GeoReferenceCounts):
            return NotImplemented
        return GeoReferenceCounts(self.generated + other.generated, self.random + other.random, None)


def js_distance(p, q):
    """Jensen-Shannon distance (log base 2) of two discrete distributions, zero entries skipped, float64."""
    def kl(a, b):
        return sum(x * math.log2(x / y) for x, y in zip(a, b) if x != 0 and y != 0)
    m = [0.5 * (x + y) for x, y in zip(p, q)]
    return math.sqrt(0.5 * kl(p, m) + 0.5 * kl(q, m))


def trigger_ids(word_map):
    """([the 8 terms' trigger ids, -1 where absent], of, the, a ids) of a word map."""
    azimuth = ["north", "south", "east", "west"]
    if "north_of" in word_map:
        azimuth = [w + "_of" for w in azimuth]
    words = ["near", "along", "across", "in"] + azimuth
    return [int(word_map.get(w, -1)) for w in words], tuple(int(word_map.get(w, -1)) for w in ("of", "the", "a"))


def _bins(bins, name):
    try:
        out = [(float(lo), float(hi)) for lo, hi in bins]
    except (TypeError, ValueError):
        raise IckError("%s must be a list of (lo, hi) pairs" % name)
    if not 1 <= len(out) <= ops.GEO_MAX_BINS:
        raise IckError("%s holds 1..%d bins" % (name, ops.GEO_MAX_BINS))
    return out


class GeoReferenceMetric:
    """m = GeoReferenceMetric(word_map, bins_distance, bins_azimuth, n_types, train_distribution, seed=0, device=None)
    c = m(tokens, image_index, entities, entity_names, row_offset=0)   # GeoReferenceCounts, no host synchronisation
    total = c1 + c2                                                    # batches add on the device
    m.result(total)        # {"generated": {term: {"n_occurrences": n, feature: JS distance, ..}}, "random": {..}}

    bins_distance / bins_azimuth: lists of (lo, hi); n_types: the number of OSM types; train_distribution: {term:
    {"distance_probs" | "azimuth_probs" | "type_probs": [..]}} as the reference's geo_probability_distr_train.pkl holds.
    tokens (N, T) int64 caption rows; image_index (N,) row -> image; entities (B, K, C) float32; entity_names
    (B, K, 52) int64; row_offset: the number of rows counted before this call (it numbers the random draws).
    result(): a term's features are near: distance; along, across, in: distance, type; north..west: azimuth; they are
    None for a term that never occurred."""

    def __init__(self, word_map, bins_distance, bins_azimuth, n_types, train_distribution, seed=0, device=None):
        if not isinstance(word_map, dict) or not word_map:
            raise IckError("word_map must be the vocabulary's dict word -> id")
        self.V = len(word_map)
        self.trigger_ids, (self.of_id, self.the_id, self.a_id) = trigger_ids(word_map)
        if not all(-1 <= i < self.V for i in self.trigger_ids + [self.of_id, self.the_id, self.a_id]):
            raise IckError("word_map must map its words to ids in [0, len(word_map))")
        self.bins_distance = _bins(bins_distance, "bins_distance")
        self.bins_azimuth = _bins(bins_azimuth, "bins_azimuth")
        if isinstance(n_types, bool) or not isinstance(n_types, int) or not 1 <= n_types <= ops.GEO_MAX_TYPES:
            raise IckError("n_types must be an int in [1, %d]" % ops.GEO_MAX_TYPES)
        self.n_types = n_types
        sizes = {"distance": len(self.bins_distance), "azimuth": len(self.bins_azimuth), "type": n_types}
        self.train = {}
        for term in TERMS:
            for feat in FEATURES[term]:
                try:
                    probs = [float(x) for x in train_distribution[term][feat + "_probs"]]
                except (KeyError, TypeError, ValueError):
                    raise IckError("train_distribution lacks %s / %s_probs" % (term, feat))
                if len(probs) != sizes[feat]:
                    raise IckError("train_distribution's %s / %s_probs has %d entries for %d bins"
                                   % (term, feat, len(probs), sizes[feat]))
                self.train[term, feat] = probs
        if isinstance(seed, bool) or not isinstance(seed, int) or not -2 ** 63 <= seed < 2 ** 64:
            raise IckError("seed must be a 64-bit int")
        self.seed = seed
        self.device = torch.device(device) if device is not None else None
        self._tables = {}

    @classmethod
    def from_reference_data(cls, directory, word_map, seed=0, device=None):
        """From the four pickles of a checkout of the reference's geo-aware/data: bins_distance.pkl, bins_azimuth.pkl,
        OSM_types_index.pkl (its length is n_types) and geo_probability_distr_train.pkl."""
        def load(name):
            with open(os.path.join(directory, name), "rb") as f:
                return pickle.load(f)
        return cls(word_map, load("bins_distance.pkl"), load("bins_azimuth.pkl"), len(load("OSM_types_index.pkl")),
                   load("geo_probability_distr_train.pkl"), seed=seed, device=device)

    def constructor_data(self):
        """The constructor's arguments but the word map, as plain data (train.Config.val_geo_metric takes it)."""
        train = {t: {f + "_probs": list(self.train[t, f]) for f in FEATURES[t]} for t in TERMS}
        return dict(bins_distance=list(self.bins_distance), bins_azimuth=list(self.bins_azimuth), n_types=self.n_types,
                    train_distribution=train, seed=self.seed)

    def _device(self, tokens):
        if self.device is not None:
            return self.device
        return tokens.device if tokens.is_cuda else torch.device("cuda", torch.cuda.current_device())

    def _bin_tables(self, dev):
        if dev not in self._tables:
            self._tables[dev] = (torch.tensor(self.bins_distance, dtype=torch.float64, device=dev),
                                 torch.tensor(self.bins_azimuth, dtype=torch.float64, device=dev))
        return self._tables[dev]

    def __call__(self, tokens, image_index, entities, entity_names, row_offset=0):
        if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.dim() != 2:
            raise IckError("tokens must be an (N, T) int64 tensor")
        if not isinstance(entities, torch.Tensor) or entities.dtype != torch.float32 or entities.dim() != 3:
            raise IckError("entities must be a (B, K, C) float32 tensor")
        if not isinstance(entity_names, torch.Tensor) or entity_names.dtype != torch.int64 or entity_names.dim() != 3:
            raise IckError("entity_names must be a (B, K, 52) int64 tensor")
        if isinstance(row_offset, bool) or not isinstance(row_offset, int) or row_offset < 0:
            raise IckError("row_offset must be an int >= 0")
        if not isinstance(image_index, torch.Tensor):
            image_index = torch.as_tensor(image_index)
        # the shape errors are raised before anything goes to the device
        N, T = tokens.shape
        if N < 1 or not 1 <= T <= ops.GEO_MAX_T:
            raise IckError("tokens: N >= 1 and 1 <= T <= %d (got %d, %d)" % (ops.GEO_MAX_T, N, T))
        B, K, Cf = entities.shape
        if B < 1 or not 1 <= K <= ops.GEO_MAX_K or Cf < 5:
            raise IckError("entities need B >= 1, 1 <= K <= %d and C >= 5 (got %s)" % (ops.GEO_MAX_K, tuple(entities.shape)))
        if tuple(entity_names.shape) != (B, K, 2 + ops.GEO_NAME_CHARS):
            raise IckError("entity_names must be (%d, %d, %d)" % (B, K, 2 + ops.GEO_NAME_CHARS))
        if tuple(image_index.shape) != (N,):
            raise IckError("image_index must be (N,)")
        dev = self._device(tokens)
        bd, ba = self._bin_tables(dev)
        return GeoReferenceCounts(*ops.geo_reference_counts(
            tokens.to(dev).contiguous(), image_index.to(dev), entities.to(dev).contiguous(),
            entity_names.to(dev).contiguous(), self.V, self.trigger_ids, self.of_id, self.the_id, self.a_id, bd, ba,
            self.n_types, seed=self.seed, row_offset=row_offset))

    def histograms(self, hist):
        """{term: {"n_occurrences": n, "distance" | "azimuth" | "type": [counts per bin]}} of one (8, W) histogram
        given as nested lists or a tensor (a tensor is read here)."""
        rows = hist.tolist() if isinstance(hist, torch.Tensor) else hist
        sizes = {"distance": len(self.bins_distance), "azimuth": len(self.bins_azimuth), "type": self.n_types}
        out = {}
        for q, term in enumerate(TERMS):
            out[term] = {"n_occurrences": int(rows[q][0])}
            for feat in FEATURES[term]:
                out[term][feat] = [int(x) for x in rows[q][_COL0[feat]:_COL0[feat] + sizes[feat]]]
        return out

    def result(self, counts):
        """The JS distances of the totals, float64 on the host (this reads the two histograms: one synchronisation)."""
        both = torch.stack([counts.generated, counts.random]).tolist()
        out = {}
        for name, hist in zip(("generated", "random"), both):
            res = {}
            for term, h in self.histograms(hist).items():
                n = h["n_occurrences"]
                res[term] = {"n_occurrences": n}
                for feat in FEATURES[term]:
                    res[term][feat] = js_distance(self.train[term, feat], [c / n for c in h[feat]]) if n else None
            out[name] = res
        return out
