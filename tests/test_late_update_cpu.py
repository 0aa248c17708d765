"""CPU: the ordering calls of functional.LateUpdate -- the record of an optimizer update that runs beside the next forward
(AdamW.overlap_next_forward) -- against fake streams and events that log ``wait_stream`` / ``record`` / ``wait_event`` / ``query``,
and its attachment to the encoders of a CPU model."""
import contextlib
import copy
import gc

import pytest
import torch

from oracle import clipvip_oracle as O


class _Stream:
    device = "gpu0"

    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev))

    def wait_stream(self, st):
        self.log.append(("wait_stream", self.name, st.name))


class _Event:
    def __init__(self, log, done=False):
        self.log, self.done = log, done

    def record(self, stream):
        self.log.append(("record", stream.name, self))

    def query(self):
        self.log.append(("query", self))
        return self.done


@pytest.fixture
def gpu(monkeypatch):
    """torch.cuda's streams and events replaced by the fakes: ``gpu.log`` lists every call, ``gpu.cur`` is the current stream,
    ``gpu.capturing[0]`` what is_current_stream_capturing() answers"""
    class G:
        log, capturing = [], [False]
    G.cur = _Stream(G.log, "cur")
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: G.cur)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: _Stream(G.log, "side"))
    monkeypatch.setattr(torch.cuda, "Event", lambda: _Event(G.log))
    monkeypatch.setattr(torch.cuda, "stream", lambda st: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: G.capturing[0])
    return G


def _pending(gpu, first_layer=2, done=False):
    from xpretrain_amd import functional as XF
    lu = XF.LateUpdate(first_layer)
    lu.event = _Event(gpu.log, done)
    return lu


def test_launch_runs_the_body_behind_the_main_stream_and_leaves_the_event(gpu):
    from xpretrain_amd import functional as XF
    lu = XF.LateUpdate(3)
    main = _Stream(gpu.log, "main")
    for _ in range(2):
        with lu.launch(main) as side:
            assert side.name == "side"
            gpu.log.append(("body",))
        ev = lu.event
        assert gpu.log == [("wait_stream", "side", "main"), ("body",), ("record", "side", ev)]
        assert lu.streams == {"gpu0": side}         # one side stream per device, made once
        del gpu.log[:]


def test_wait_touches_streams_only_at_the_first_late_layer_and_only_while_pending(gpu):
    from xpretrain_amd import functional as XF
    lu = XF.LateUpdate(2)
    for li in range(4):
        lu.wait(li)
    assert gpu.log == []                            # nothing pending
    lu = _pending(gpu, 2)
    for li in (0, 1, 3):
        lu.wait(li)
    assert gpu.log == []
    lu.wait(2)
    assert gpu.log == [("wait_event", "cur", lu.event)]
    del gpu.log[:]
    a, b = _Stream(gpu.log, "a"), _Stream(gpu.log, "b")
    lu.wait(2, a, b)
    assert gpu.log == [("wait_event", "a", lu.event), ("wait_event", "b", lu.event)] and lu.event is not None


def test_join_forgets_a_finished_update_and_waits_for_an_unfinished_one(gpu):
    lu = _pending(gpu, done=True)
    ev = lu.event
    lu.join()
    assert lu.event is None and gpu.log == [("query", ev)]
    lu.join()
    assert gpu.log == [("query", ev)]
    del gpu.log[:]
    lu = _pending(gpu, done=False)
    ev = lu.event
    lu.join()
    assert lu.event is ev and gpu.log == [("query", ev), ("wait_event", "cur", ev)]


def test_a_capturing_stream_neither_queries_nor_waits(gpu):
    gpu.capturing[0] = True
    for done in (False, True):
        lu = _pending(gpu, 2, done)
        ev = lu.event
        lu.wait(2)
        lu.wait(2, _Stream(gpu.log, "a"))
        lu.join()
        assert gpu.log == [] and lu.event is ev


def test_join_late_weights_joins_every_live_record(gpu):
    from xpretrain_amd import functional as XF
    a, b = _pending(gpu, 1, done=True), _pending(gpu, 2, done=False)
    eb = b.event
    XF.join_late_weights()
    assert a.event is None and b.event is eb and ("wait_event", "cur", eb) in gpu.log
    assert {a, b} <= set(XF._LATE_UPDATES)
    gc.collect()
    ref = len(XF._LATE_UPDATES)
    del a
    gc.collect()
    assert len(XF._LATE_UPDATES) == ref - 1 and b in XF._LATE_UPDATES
    del gpu.log[:]
    XF.join_late_weights()
    assert gpu.log == [("query", eb), ("wait_event", "cur", eb)]


def test_the_old_names_are_gone():
    from xpretrain_amd import functional as XF
    assert not hasattr(XF, "LATE_WEIGHTS") and not hasattr(XF, "wait_late_weights")


# ------------------------------------------------------------------------------------------ attachment (a CPU model: no stream is touched)
class _Args:
    clip_config = O.hf_config_dict(128, 2, 4, 256, 16, 32, 128, 2, 4, 256, 120, 16, 64)
    clip_weights = ""
    clip_vision_additional_config = dict(type="ViP", temporal_size=2, if_use_temporal_embed=1, logit_scale_init_value=4.6, add_cls_num=3)


def _model():
    from xpretrain_amd.modeling import VidCLIP
    model = VidCLIP(_Args())
    return model, [m for m in model.modules() if type(m).__name__ == "CLIPEncoder"]


def test_overlap_next_forward_attaches_replaces_and_detaches():
    from xpretrain_amd.optimization import AdamW
    model, encs = _model()
    assert len(encs) == 2 and all(e.late_update is None for e in encs)
    opt = AdamW(model.parameters(), lr=1e-4)
    opt.overlap_next_forward(model, 2)
    lu = encs[0].late_update
    assert lu is not None and lu is encs[1].late_update and lu.first_layer == 2 and lu.event is None
    assert opt._late[1] == 2 and opt._late[0] == frozenset(id(p) for e in encs for l in e.layers[2:] for p in l.parameters())
    assert copy.deepcopy(encs[0]).late_update is None       # a copy's parameters are nobody's late parameters
    opt.overlap_next_forward(model, 1)              # the same optimizer again: its own record is replaced
    lu1 = encs[0].late_update
    assert lu1 is not lu and lu1 is encs[1].late_update and lu1.first_layer == 1 and opt._late[1] == 1
    opt.overlap_next_forward(model, None)
    assert all(e.late_update is None for e in encs) and opt._late is None


def test_only_encoders_with_a_late_parameter_of_this_optimizer_are_attached():
    from xpretrain_amd.optimization import AdamW
    model, encs = _model()
    opt = AdamW(encs[0].parameters(), lr=1e-4)
    opt.overlap_next_forward(model, 3)
    assert encs[0].late_update is not None and encs[1].late_update is None
    opt.overlap_next_forward(model, 4)              # no layer >= 4 in a tower of four
    assert encs[0].late_update is None and opt._late is None


def test_a_second_optimizer_on_an_occupied_encoder_is_refused():
    from xpretrain_amd.optimization import AdamW
    model, encs = _model()
    first, second = AdamW(model.parameters(), lr=1e-4), AdamW(model.parameters(), lr=1e-4)
    first.overlap_next_forward(model, 2)
    lu = encs[0].late_update
    with pytest.raises(ValueError):
        second.overlap_next_forward(model, 1)
    assert all(e.late_update is lu for e in encs) and second._late is None      # nothing changed
    first.overlap_next_forward(model, None)
    second.overlap_next_forward(model, 1)
    assert all(e.late_update is not None and e.late_update.first_layer == 1 for e in encs)
    del second                                      # a dead optimizer's record does not occupy the encoder
    gc.collect()
    first.overlap_next_forward(model, 2)
    assert all(e.late_update.first_layer == 2 for e in encs)
