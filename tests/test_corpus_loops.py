"""How far the corpus folds and test loops of training.py get before they refuse: search_shards,
search_window_shards, search_shards_weighted, search_window_shards_weighted, search_shards_prefiltered and the six test_model_corpus*
loops, driven on the host with a recording stub in place of the model.  Every case is a refusal that comes before the first launch:
its type, its whole text, and the stub's calls up to it -- which pins that the k and Q checks precede any retrieval, that a shard of
videos is encoded before its duration is checked and a shard of windows after, that the one-shard check of test_model_corpus precedes
its k check, and that gt_video is checked against the corpus once the shards are folded.  Also: search_shards encodes without a shard's
cell_counts, every other fold with them.  No device, no kernel, no tolerance."""
import numpy as np
import pytest
import torch

Q = 4
GT_VIDEO = [2, 0, 3, 1]
GT_TIMES = [[1.0, 2.0]] * Q
QUERIES = dict(query_features=torch.zeros(Q, 5, 300), query_mask=torch.ones(Q, 5, 1, dtype=torch.uint8))
LOOPS = ("test_model_corpus", "test_model_corpus_windows", "test_model_corpus_window_shards", "test_model_corpus_weighted_shards",
         "test_model_corpus_window_shards_weighted", "test_model_corpus_prefiltered_shards")
FOLDS = ("search_shards", "search_window_shards", "search_shards_weighted", "search_window_shards_weighted", "search_shards_prefiltered")


class Bank:
    device = torch.device("cpu")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class Stub:
    """the model's retrieval surface: every call is logged as (name, keyword arguments) and answers with a placeholder"""
    L = 8

    def __init__(self):
        self.calls = []

    def names(self):
        return [name for name, _ in self.calls]

    def eval(self):
        return self

    def _log(self, name, kw, out):
        self.calls.append((name, kw))
        return out

    def encode_queries(self, query_features, query_mask, **kw):
        return self._log("encode_queries", kw, "query bank")

    def encode_videos(self, video_features, video_mask, length_mask, moment_mask, **kw):
        return self._log("encode_videos", kw, Bank(len(video_features)))

    def encode_windows(self, raw, lengths, **kw):
        return self._log("encode_windows", kw, Bank(len(lengths)))

    def search(self, bank, queries, **kw):
        return self._log("search", kw, {"gt_rank": None})

    def search_windows(self, bank, queries, **kw):
        return self._log("search_windows", kw, {"gt_rank": None})

    def new_survivors(self, queries, prefilter, tau):
        return self._log("new_survivors", {}, "survivors")

    def fold_survivors(self, survivors, bank, queries):
        return self._log("fold_survivors", {}, None)

    def search_survivors(self, survivors, queries, **kw):
        return self._log("search_survivors", kw, {"prefilter_gt_rank": None})


class Meter:
    """stands in for a CorpusMeter (or a VideoRankMeter): the loops read ``n`` before anything runs"""

    def __init__(self, n=(1, 5)):
        self.n = n


def video_shard(n, durations=None):
    return dict(video_features=np.zeros((n, 16, 24), np.float32), video_mask=None, length_mask=None, moment_mask=None,
                duration=[10.0] * (n if durations is None else durations), cell_counts=[36] * n)


def window_shard(n, durations=None):
    return dict(raw=None, lengths=[20] * n, duration=[10.0] * (n if durations is None else durations))


def shards_for(name, split, short=None):
    """shards of ``split`` videos in the form ``name`` takes; shard ``short`` carries one duration too few"""
    make = window_shard if "window" in name else video_shard
    return [make(n, n - 1 if i == short else None) for i, n in enumerate(split)]


def training():
    import models
    return models.vml_amd.training


def run_loop(name, stub, split=(2, 3), short=None, gt_video=GT_VIDEO, gt_times=GT_TIMES, meter=None, **kw):
    f = getattr(training(), name)
    shards = shards_for(name, split, short)
    if name == "test_model_corpus_windows":
        lengths, duration = sum((s["lengths"] for s in shards), []), sum((s["duration"] for s in shards), [])
        return f(stub, None, lengths, QUERIES, gt_video, gt_times, duration, meter, **kw)
    if name == "test_model_corpus_prefiltered_shards":
        kw.setdefault("prefilter", 3)
    return f(stub, shards, QUERIES, gt_video, gt_times, meter, **kw)


def run_fold(name, stub, split=(2, 3), short=None, **kw):
    if name == "search_shards_prefiltered":
        kw.setdefault("prefilter", 3)
    return getattr(training(), name)(stub, shards_for(name, split, short), "query bank", **kw)


def refused(run, name, message, calls, **kw):
    stub = Stub()
    with pytest.raises(ValueError) as e:
        run(name, stub, **kw)
    assert type(e.value) is ValueError
    assert str(e.value) == message
    assert stub.names() == calls
    return stub


# ---------------------------------------------------------------- the k and Q checks: before anything runs
K_SMALL = {
    "test_model_corpus":
        ("test_model_corpus: k = 3 entries per query cannot give an exact R@5 / VR@5 at k_video = 1: needs k >= max(n) * k_video = 5",
         "test_model_corpus: k = 25 entries per query cannot give an exact R@10 / VR@10 at k_video = 5: needs k >= max(n) * k_video = 50",
         "test_model_corpus: k = 24 entries per query cannot give an exact R@5 / VR@5 at k_video = 5: needs k >= max(n) * k_video = 25"),
    "test_model_corpus_windows":
        ("test_model_corpus_windows: k = 3 entries per query cannot give an exact R@5 / VR@5 at k_video = 1: needs k >= max(n) * k_video = 5",
         "test_model_corpus_windows: k = 25 entries per query cannot give an exact R@10 / VR@10 at k_video = 5: needs k >= max(n) * k_video = 50",
         "test_model_corpus_windows: k = 24 entries per query cannot give an exact R@5 / VR@5 at k_video = 5: needs k >= max(n) * k_video = 25"),
    "test_model_corpus_window_shards":
        ("test_model_corpus_window_shards: k = 3 entries per query cannot give an exact R@5 / VR@5 at k_video = 1: "
         "needs k >= max(n) * k_video = 5",
         "test_model_corpus_window_shards: k = 25 entries per query cannot give an exact R@10 / VR@10 at k_video = 5: "
         "needs k >= max(n) * k_video = 50",
         "test_model_corpus_window_shards: k = 24 entries per query cannot give an exact R@5 / VR@5 at k_video = 5: "
         "needs k >= max(n) * k_video = 25"),
    "test_model_corpus_weighted_shards":
        ("test_model_corpus_weighted_shards: k = 3 entries per query cannot give an exact R@5 / VR@5 at k_video = 1: "
         "needs k >= max(n) * k_video = 5",
         "test_model_corpus_weighted_shards: k = 25 entries per query cannot give an exact R@10 / VR@10 at k_video = 5: "
         "needs k >= max(n) * k_video = 50",
         "test_model_corpus_weighted_shards: k = 24 entries per query cannot give an exact R@5 / VR@5 at k_video = 5: "
         "needs k >= max(n) * k_video = 25"),
    "test_model_corpus_window_shards_weighted":
        ("test_model_corpus_window_shards_weighted: k = 3 entries per query cannot give an exact R@5 / VR@5 at k_video = 1: "
         "needs k >= max(n) * k_video = 5",
         "test_model_corpus_window_shards_weighted: k = 25 entries per query cannot give an exact R@10 / VR@10 at k_video = 5: "
         "needs k >= max(n) * k_video = 50",
         "test_model_corpus_window_shards_weighted: k = 24 entries per query cannot give an exact R@5 / VR@5 at k_video = 5: "
         "needs k >= max(n) * k_video = 25"),
    "test_model_corpus_prefiltered_shards":
        ("test_model_corpus_prefiltered_shards: k = 3 entries per query cannot give an exact R@5 / VR@5 at k_video = 1: "
         "needs k >= max(n) * k_video = 5",
         "test_model_corpus_prefiltered_shards: k = 25 entries per query cannot give an exact R@10 / VR@10 at k_video = 5: "
         "needs k >= max(n) * k_video = 50",
         "test_model_corpus_prefiltered_shards: k = 24 entries per query cannot give an exact R@5 / VR@5 at k_video = 5: "
         "needs k >= max(n) * k_video = 25"),
}


@pytest.mark.parametrize("name", LOOPS)
def test_k_too_small(name):
    below_n, below_n_videos, default_meter = K_SMALL[name]
    refused(run_loop, name, below_n, [], meter=Meter((1, 5)), k=3, k_video=1)                  # k < max(meter.n)
    refused(run_loop, name, below_n_videos, [], meter=Meter((1, 10)), k=25, k_video=5)         # k < max(meter.n) * k_video
    refused(run_loop, name, default_meter, [], meter=None, k=24, k_video=5)                    # no meter: the default one's n = (1, 5)


Q_MISMATCH = {
    "test_model_corpus":
        ("test_model_corpus: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (3,), (4, 2))",
         "test_model_corpus: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (4,), (5, 2))"),
    "test_model_corpus_windows":
        ("test_model_corpus_windows: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (3,), (4, 2))",
         "test_model_corpus_windows: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (4,), (5, 2))"),
    "test_model_corpus_window_shards":
        ("test_model_corpus_window_shards: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (3,), (4, 2))",
         "test_model_corpus_window_shards: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (4,), (5, 2))"),
    "test_model_corpus_weighted_shards":
        ("test_model_corpus_weighted_shards: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (3,), (4, 2))",
         "test_model_corpus_weighted_shards: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (4,), (5, 2))"),
    "test_model_corpus_window_shards_weighted":
        ("test_model_corpus_window_shards_weighted: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (3,), (4, 2))",
         "test_model_corpus_window_shards_weighted: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (4,), (5, 2))"),
    "test_model_corpus_prefiltered_shards":
        ("test_model_corpus_prefiltered_shards: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (3,), (4, 2))",
         "test_model_corpus_prefiltered_shards: gt_video (Q,) and gt_times (Q, 2) must cover the Q = 4 queries (got (4,), (5, 2))"),
}


@pytest.mark.parametrize("name", LOOPS)
def test_ground_truth_must_cover_the_queries(name):
    short_video, long_times = Q_MISMATCH[name]
    refused(run_loop, name, short_video, [], meter=Meter(), gt_video=GT_VIDEO[:3])
    refused(run_loop, name, long_times, [], meter=Meter(), gt_times=GT_TIMES + [[0.0, 1.0]])
    refused(run_loop, name, K_SMALL[name][0], [], meter=Meter(), gt_video=GT_VIDEO[:3], k=3, k_video=1)          # the k check comes first


# ---------------------------------------------------------------- test_model_corpus: the video-level options need one shard
ONE_SHARD = ("test_model_corpus: video_weight / max_videos / video_meter need the corpus as one shard (got %d): the video weight and rank "
             "are corpus-wide, and the plain shard merges do not carry them (test_model_corpus_weighted_shards does)")


@pytest.mark.parametrize("option", [dict(video_weight=0.5), dict(max_videos=2), dict(video_meter=Meter())], ids=lambda o: next(iter(o)))
def test_video_level_options_need_one_shard(option):
    assert ONE_SHARD % 2 == ("test_model_corpus: video_weight / max_videos / video_meter need the corpus as one shard (got 2): the video "
                             "weight and rank are corpus-wide, and the plain shard merges do not carry them "
                             "(test_model_corpus_weighted_shards does)")
    refused(run_loop, "test_model_corpus", ONE_SHARD % 2, [], meter=Meter(), split=(2, 3), **option)
    refused(run_loop, "test_model_corpus", ONE_SHARD % 3, [], meter=Meter(), split=(2, 2, 1), **option)
    refused(run_loop, "test_model_corpus", ONE_SHARD % 0, [], meter=Meter(), split=(), **option)
    refused(run_loop, "test_model_corpus", ONE_SHARD % 2, [], meter=Meter(), split=(2, 3), k=3, k_video=1, **option)   # before the k check


# ---------------------------------------------------------------- a shard's duration: videos after the encode, windows before
def test_short_duration_in_the_folds():
    s = refused(run_fold, "search_shards", "search_shards: duration must cover the shard's 2 videos (got 1)", ["encode_videos"], short=0)
    assert s.calls == [("encode_videos", {})]                                           # without the shard's cell_counts
    s = refused(run_fold, "search_shards_weighted", "search_shards_weighted: duration must cover the shard's 2 videos (got 1)",
                ["encode_videos"], short=0)
    assert s.calls == [("encode_videos", {"cell_counts": [36, 36]})]                    # with them
    s = refused(run_fold, "search_shards_prefiltered", "search_shards_prefiltered: duration must cover the shard's 2 videos (got 1)",
                ["new_survivors", "encode_videos"], short=0)
    assert s.calls[1] == ("encode_videos", {"cell_counts": [36, 36]})
    refused(run_fold, "search_window_shards", "search_window_shards: duration must cover the shard's 2 videos (got 1)", [], short=0)
    refused(run_fold, "search_window_shards_weighted", "search_window_shards_weighted: duration must cover the shard's 2 videos (got 1)", [],
            short=0)


def test_short_duration_in_the_loops():
    """the message names the fold that walks the shards; the queries are encoded by then"""
    m = Meter()
    s = refused(run_loop, "test_model_corpus", "search_shards: duration must cover the shard's 2 videos (got 1)",
                ["encode_queries", "encode_videos"], meter=m, short=0)
    assert s.calls[1] == ("encode_videos", {})
    for option in (dict(video_weight=0.5), dict(max_videos=2), dict(video_meter=Meter())):
        s = refused(run_loop, "test_model_corpus", "test_model_corpus: duration must cover the shard's 5 videos (got 4)",
                    ["encode_queries", "encode_videos"], meter=m, split=(5,), short=0, **option)
        assert s.calls[1] == ("encode_videos", {"cell_counts": [36] * 5})
    refused(run_loop, "test_model_corpus_window_shards", "search_window_shards: duration must cover the shard's 2 videos (got 1)",
            ["encode_queries"], meter=m, short=0)
    refused(run_loop, "test_model_corpus_weighted_shards", "search_shards_weighted: duration must cover the shard's 2 videos (got 1)",
            ["encode_queries", "encode_videos"], meter=m, short=0)
    refused(run_loop, "test_model_corpus_window_shards_weighted",
            "search_window_shards_weighted: duration must cover the shard's 2 videos (got 1)", ["encode_queries"], meter=m, short=0)
    refused(run_loop, "test_model_corpus_prefiltered_shards", "search_shards_prefiltered: duration must cover the shard's 2 videos (got 1)",
            ["encode_queries", "new_survivors", "encode_videos"], meter=m, short=0)


def test_short_duration_in_a_later_shard():
    """the first shard is searched and taken as it is, the second one refused: after its encode for videos, before it for windows"""
    refused(run_fold, "search_shards", "search_shards: duration must cover the shard's 3 videos (got 2)",
            ["encode_videos", "search", "encode_videos"], short=1)
    refused(run_fold, "search_window_shards", "search_window_shards: duration must cover the shard's 3 videos (got 2)",
            ["encode_windows", "search_windows"], short=1)
    refused(run_fold, "search_shards_prefiltered", "search_shards_prefiltered: duration must cover the shard's 3 videos (got 2)",
            ["new_survivors", "encode_videos", "fold_survivors", "encode_videos"], short=1)


# ---------------------------------------------------------------- no shard at all
def test_empty_corpus():
    refused(run_fold, "search_shards", "search_shards: at least one shard of videos", [], split=())
    refused(run_fold, "search_window_shards", "search_window_shards: at least one shard of videos", [], split=())
    refused(run_fold, "search_shards_weighted", "search_shards_weighted: at least one shard of videos", [], split=())
    refused(run_fold, "search_window_shards_weighted", "search_window_shards_weighted: at least one shard of videos", [], split=())
    refused(run_fold, "search_shards_prefiltered", "search_shards_prefiltered: at least one shard of videos", ["new_survivors"], split=())
    m = Meter()
    refused(run_loop, "test_model_corpus", "search_shards: at least one shard of videos", ["encode_queries"], meter=m, split=())
    refused(run_loop, "test_model_corpus_window_shards", "search_window_shards: at least one shard of videos", ["encode_queries"], meter=m,
            split=())
    refused(run_loop, "test_model_corpus_weighted_shards", "search_shards_weighted: at least one shard of videos", ["encode_queries"],
            meter=m, split=())
    refused(run_loop, "test_model_corpus_window_shards_weighted", "search_window_shards_weighted: at least one shard of videos",
            ["encode_queries"], meter=m, split=())
    refused(run_loop, "test_model_corpus_prefiltered_shards", "search_shards_prefiltered: at least one shard of videos",
            ["encode_queries", "new_survivors"], meter=m, split=())


# ---------------------------------------------------------------- gt_video against the corpus
def test_windows_loop_duration_and_gt_video():
    """one message for both, before anything runs"""
    message = "test_model_corpus_windows: duration must be (V,) = (5,) seconds and gt_video lie in [0, 5) (got (%d,))"
    refused(run_loop, "test_model_corpus_windows", message % 5, [], meter=Meter(), gt_video=[2, 0, 5, 1])
    refused(run_loop, "test_model_corpus_windows", message % 5, [], meter=Meter(), gt_video=[2, -1, 3, 1])
    refused(run_loop, "test_model_corpus_windows", message % 4, [], meter=Meter(), short=1)
    assert message % 4 == "test_model_corpus_windows: duration must be (V,) = (5,) seconds and gt_video lie in [0, 5) (got (4,))"


def test_gt_video_out_of_range():
    """with a video-level option test_model_corpus checks its one shard before the search; the sharded loops check once the fold is done
    (one shard here: its list is taken as it is, so the stub's placeholder reaches the check)"""
    m = Meter()
    for option in (dict(video_weight=0.5), dict(max_videos=2), dict(video_meter=Meter())):
        refused(run_loop, "test_model_corpus", "test_model_corpus: gt_video must lie in [0, 3), the videos of the shard",
                ["encode_queries", "encode_videos"], meter=m, split=(3,), gt_video=[2, 0, 3, 1], **option)
    refused(run_loop, "test_model_corpus", "test_model_corpus: gt_video must lie in [0, 3), the videos of the shards",
            ["encode_queries", "encode_videos", "search"], meter=m, split=(3,), gt_video=[2, 0, 3, 1])
    refused(run_loop, "test_model_corpus", "test_model_corpus: gt_video must lie in [0, 5), the videos of the shards",
            ["encode_queries", "encode_videos", "search"], meter=m, split=(5,), gt_video=[2, -1, 3, 1])
    refused(run_loop, "test_model_corpus_window_shards", "test_model_corpus_window_shards: gt_video must lie in [0, 3), the videos of the shards",
            ["encode_queries", "encode_windows", "search_windows"], meter=m, split=(3,), gt_video=[2, 0, 3, 1])
    refused(run_loop, "test_model_corpus_prefiltered_shards",
            "test_model_corpus_prefiltered_shards: gt_video must lie in [0, 4), the videos of the shards",
            ["encode_queries", "new_survivors", "encode_videos", "fold_survivors", "encode_videos", "fold_survivors", "search_survivors"],
            meter=m, split=(3, 1), gt_video=[2, 0, 4, 1])


# ---------------------------------------------------------------- what the folds hand on
def test_one_shard_is_taken_as_it_is():
    """a plain fold of one shard returns that shard's list and its host arrays, with the caller's options at the search"""
    stub = Stub()
    carry, duration = run_fold("search_shards", stub, split=(3,), k=7, k_video=2, nms_thresh=0.25, max_batch=8)
    assert carry == {"gt_rank": None} and duration.dtype == np.float64 and duration.tolist() == [10.0] * 3
    assert stub.calls == [("encode_videos", {}), ("search", dict(k=7, k_video=2, nms_thresh=0.25, max_batch=8))]
    stub = Stub()
    carry, duration, n_rows = run_fold("search_window_shards", stub, split=(3,), window=16, stride=4, k=7, k_video=2, k_window=3, nms_thresh=0.25,
                                       max_batch=8)
    assert carry == {"gt_rank": None} and duration.tolist() == [10.0] * 3 and n_rows.dtype == np.int64 and n_rows.tolist() == [20] * 3
    assert stub.calls == [("encode_windows", dict(window=16, stride=4, max_batch=8)),
                          ("search_windows", dict(k=7, k_video=2, k_window=3, nms_thresh=0.25, max_batch=8))]
    stub = Stub()
    carry, duration = run_fold("search_shards_prefiltered", stub, split=(2, 3), k=7, k_video=2, nms_thresh=0.25, max_batch=8, max_videos=2,
                               gt_video=GT_VIDEO)
    assert carry == {"prefilter_gt_rank": None} and duration.tolist() == [10.0] * 5
    assert stub.names() == ["new_survivors", "encode_videos", "fold_survivors", "encode_videos", "fold_survivors", "search_survivors"]
    assert stub.calls[-1][1] == dict(k=7, k_video=2, nms_thresh=0.25, max_batch=8, video_weight=None, max_videos=2, n_videos=None,
                                     gt_video=GT_VIDEO)
