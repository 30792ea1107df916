"""wave_tasks.ArenaTask and finish_modules without a GPU: what the record knows about itself
(fan-in, selection) and the order of the batched aggregates' epilogue, which release_early relies on."""
from __future__ import annotations

import pytest
import torch
from torch import nn

from dasklearn_amd import wave_tasks
from dasklearn_amd.arena import input_arenas
from dasklearn_amd.wave_tasks import ArenaTask, finish_modules


def test_fan_in_from_views_from_rows_and_from_neither():
    views = {torch.float32: [None] * 5, torch.bfloat16: [None] * 5}
    assert ArenaTask(None, None, views).fan_in == 5
    assert ArenaTask(None, None, views, None, [[]] * 7).fan_in == 5  # the views say it first
    assert ArenaTask(None, None, {}, None, [[], [], []]).fan_in == 3
    with pytest.raises(ValueError, match="a task without parameters and without rows does not state its fan-in"):
        ArenaTask(None, None, {}).fan_in
    assert ArenaTask(None, None, {}).rows is None and ArenaTask(None, None, {}).weights is None
    assert not hasattr(ArenaTask(None, None, {}), "__dict__")


def test_select_keeps_model0_and_layout_and_picks_by_index():
    ms = [nn.Linear(3, 2) for _ in range(4)]
    layout, params, _ = input_arenas(ms)
    a, b = [object() for _ in range(4)], [object() for _ in range(4)]
    task = ArenaTask(ms[0], layout, {torch.float32: a, torch.bfloat16: b}, [0.25] * 4, params)
    sel = task.select([1, 3], [0.5, 0.5])
    assert sel.model0 is ms[0] and sel.layout is layout and sel.weights == [0.5, 0.5]
    assert list(sel.views) == [torch.float32, torch.bfloat16]
    assert sel.views[torch.float32] == [a[1], a[3]] and sel.views[torch.bfloat16] == [b[1], b[3]]
    assert len(sel.rows) == 2 and sel.rows[0] is params[1] and sel.rows[1] is params[3]
    assert sel.fan_in == 2 and task.fan_in == 4 and task.weights == [0.25] * 4  # the task itself is only read
    assert ArenaTask(ms[0], layout, {torch.float32: a}).select([2], [1.0]).rows is None


def _recorded_finish(monkeypatch, on_launched, restride=False):
    """finish_modules over three tasks with a module builder that records, per module, what
    `prepared` held and what had happened when it was built."""
    events = []
    tasks = [ArenaTask(f"model{i}", f"layout{i}", {}) for i in range(3)]
    prepared = list(tasks)

    def build(model0, layout, arenas):
        events.append(("module", model0, layout, arenas, [t is None for t in prepared]))
        return "mod:" + model0
    monkeypatch.setattr(wave_tasks, "module_from_arenas", build)
    monkeypatch.setattr(wave_tasks, "_restride", lambda mod, layout: events.append(("restride", mod, layout)) or mod)
    outs = ["o0", "o1", "o2"]
    launched = (lambda: events.append(("launched", list(prepared)))) if on_launched else None
    mods = finish_modules(prepared, outs, launched, restride)
    return tasks, prepared, events, mods


def test_finish_modules_calls_on_launched_once_before_the_first_module(monkeypatch):
    tasks, prepared, events, mods = _recorded_finish(monkeypatch, True)
    assert [e[0] for e in events] == ["launched", "module", "module", "module"]
    assert events[0][1] == tasks  # nothing consumed yet when the inputs are released
    assert mods == ["mod:model0", "mod:model1", "mod:model2"]
    assert [e[1:4] for e in events[1:]] == [(f"model{i}", f"layout{i}", f"o{i}") for i in range(3)]
    _, _, events, mods = _recorded_finish(monkeypatch, False)  # no callback: the modules alone
    assert [e[0] for e in events] == ["module"] * 3 and len(mods) == 3


def test_finish_modules_drops_each_task_as_soon_as_its_module_exists(monkeypatch):
    _, prepared, events, _ = _recorded_finish(monkeypatch, True)
    built = [e[4] for e in events if e[0] == "module"]
    # when module i is built, entries 0..i are gone (so entry i is by the time module i+1 is built), the later ones are not
    assert built == [[True, False, False], [True, True, False], [True, True, True]]
    assert prepared == [None, None, None]


def test_finish_modules_restrides_only_on_request(monkeypatch):
    _, _, events, _ = _recorded_finish(monkeypatch, True)
    assert not [e for e in events if e[0] == "restride"]
    _, _, events, mods = _recorded_finish(monkeypatch, True, restride=True)
    assert [e[0] for e in events] == ["launched", "module", "restride", "module", "restride", "module", "restride"]
    assert [e[1:] for e in events if e[0] == "restride"] == [(f"mod:model{i}", f"layout{i}") for i in range(3)]
