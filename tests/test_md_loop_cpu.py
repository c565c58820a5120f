"""CPU checks of the schedule of `_driver.md_loop`, the run loop under the eight drivers that integrate, and of
`dynamics.langevin_warm_up`: a fake batch and a fake state append (name, k, finish_only) to one list, and every case asserts the exact
sequence of evaluations, integrator calls, hooks and log rows.  No library and no device."""
import numpy as np

from torch_m3gnet import _driver, dynamics
from torch_m3gnet.data import MaterialGraphKey as K


class Recorder:
    """The batch and the state in one: `evaluate` hands out a fresh dict per step k, `step` records which forces it was given."""

    def __init__(self):
        self.calls, self.k, self.whole, self.pos = [], -1, None, "pos"

    def evaluate(self, pos, into):
        assert pos is self.pos
        self.k += 1
        self.calls.append(("evaluate", self.k, None))
        return {K.FORCES: ("forces", self.k), K.STRESSES: ("stresses", self.k), K.TOTAL_ENERGY: ("energies", self.k)}

    def step(self, forces, finish_only, second=None):
        assert isinstance(finish_only, bool) and second == ("stresses", self.k)
        self.calls.append(("step" if forces == ("forces", self.k) else forces, self.k, finish_only))

    def log(self, j, out):
        assert out[K.TOTAL_ENERGY] == ("energies", self.k)
        self.calls.append(("log", j, None))


def plain(k, last):
    return [("evaluate", k, None), ("step", k, k == last)]


def test_no_steps_is_one_evaluation_one_finish_and_one_row():
    r = Recorder()
    out = _driver.md_loop(r, r, 0, log=r.log, loginterval=2)
    assert r.calls == [("evaluate", 0, None), ("step", 0, True), ("log", 0, None)]
    assert out[K.FORCES] == ("forces", 0)   # the last evaluation is returned


def test_rows_at_the_multiples_of_loginterval_and_at_the_last_step():
    r = Recorder()
    _driver.md_loop(r, r, 1, log=r.log, loginterval=2)
    assert r.calls == plain(0, 1) + [("log", 0, None)] + plain(1, 1) + [("log", 1, None)]
    r = Recorder()
    _driver.md_loop(r, r, 3, log=r.log, loginterval=2)
    assert r.calls == (plain(0, 3) + [("log", 0, None)] + plain(1, 3) + plain(2, 3) + [("log", 2, None)] + plain(3, 3)
                       + [("log", 3, None)])
    assert [c for c in r.calls if c[2]] == [("step", 3, True)]   # finish_only at the last step only
    r = Recorder()
    _driver.md_loop(r, r, 2)   # no log: nothing but evaluations and steps
    assert r.calls == plain(0, 2) + plain(1, 2) + plain(2, 2)


def test_synchronous_point_inside_the_run_finishes_acts_restarts_then_logs():
    r = Recorder()

    def act(k, out):
        r.calls.append(("act", k, None))
        return lambda: r.calls.append(("resumed", k, None))

    _driver.md_loop(r, r, 3, log=r.log, sync_at=lambda k: k == 2, at_sync=act)
    assert r.calls == (plain(0, 3) + [("log", 0, None)] + plain(1, 3) + [("log", 1, None)]
                       + [("evaluate", 2, None), ("step", 2, True), ("act", 2, None), ("step", 2, False), ("resumed", 2, None),
                          ("log", 2, None)] + plain(3, 3) + [("log", 3, None)])


def test_synchronous_point_at_the_last_step_does_not_restart():
    r = Recorder()
    _driver.md_loop(r, r, 2, sync_at=lambda k: k > 0, at_sync=lambda k, out: r.calls.append(("act", k, None)))
    assert r.calls == (plain(0, 2) + [("evaluate", 1, None), ("step", 1, True), ("act", 1, None), ("step", 1, False)]
                       + [("evaluate", 2, None), ("step", 2, True), ("act", 2, None)])


def test_before_hook_runs_between_evaluation_and_step_and_may_substitute_the_forces():
    r = Recorder()

    def before(k, out, logged):
        r.calls.append(("before", k, logged))
        return "biased" if k == 1 else None

    def after(k, out):
        r.calls.append(("after", k, None))

    _driver.md_loop(r, r, 2, log=r.log, loginterval=2, before=before, after=after)
    assert r.calls == [("evaluate", 0, None), ("before", 0, True), ("step", 0, False), ("log", 0, None), ("after", 0, None),
                       ("evaluate", 1, None), ("before", 1, False), ("biased", 1, False), ("after", 1, None),
                       ("evaluate", 2, None), ("before", 2, True), ("step", 2, True), ("log", 2, None), ("after", 2, None)]


def test_first_logged_step_numbers_the_rows_from_the_end_of_the_equilibration():
    r = Recorder()
    _driver.md_loop(r, r, 2 + 3, log=r.log, loginterval=2, first_logged=2)   # equilibration 2, steps 3
    assert [c for c in r.calls if c[0] == "log"] == [("log", 0, None), ("log", 2, None), ("log", 3, None)]
    at = r.calls.index(("log", 0, None))
    assert r.calls[at - 1] == ("step", 2, False) and not any(c[0] == "log" for c in r.calls[:at])   # no row for k < equilibration
    assert r.calls[-1] == ("log", 3, None) and r.calls[-2] == ("step", 5, True)


def test_other_second_inputs_and_buffers():
    class Energies(Recorder):
        def step(self, forces, finish_only, second=None):
            self.calls.append((second, self.k, finish_only))

    r = Energies()
    _driver.md_loop(r, r, 1, K.TOTAL_ENERGY)   # (`ti_step`: the energies)
    assert [c for c in r.calls if c[0] != "evaluate"] == [(("energies", 0), 0, False), (("energies", 1), 1, True)]
    r = Energies()
    _driver.md_loop(r, r, 0, None)             # (`pimd_step`: none)
    assert r.calls[-1] == (None, 0, True)
    seen = []
    r = Recorder()
    r.whole, evaluate = "whole", r.evaluate
    r.evaluate = lambda pos, into: (seen.append(into), evaluate(pos, into))[1]
    _driver.md_loop(r, r, 0)
    _driver.md_loop(r, r, 0, into="mine")
    assert seen == ["whole", "mine"]


def test_warm_up_is_equilibration_plus_one_evaluations_ending_on_a_finish(monkeypatch):
    made = []

    class FakeState(Recorder):
        def __init__(self, pos, lattice, offsets, masses, velocities, temperatures, seeds, ensemble, **common):
            super().__init__()
            self.args = dict(pos=pos, lattice=lattice, masses=masses, velocities=velocities, temperatures=temperatures, seeds=seeds,
                             ensemble=ensemble, **common)
            made.append(self)

        def step(self, forces, finish_only, second=None):
            self.calls.append((forces, second, finish_only))

    class Batch(Recorder):
        lattice, offsets, device = "lattice", np.array([0, 2, 5]), "cpu"

    monkeypatch.setattr(dynamics, "DynState", FakeState)
    batch, masses, seeds = Batch(), [np.full(2, 63.5), np.full(3, 197.0)], np.array([3, 4], dtype=np.uint64)
    batch.step = None   # (the warm-up steps the state it makes, not the batch)
    warm = dynamics.langevin_warm_up(batch, masses, 300.0, seeds, 3, dt=2.0, friction=0.02)
    assert made == [warm] and warm.args["ensemble"] == "nvt_langevin" and (warm.args["dt"], warm.args["friction"]) == (2.0, 0.02)
    assert warm.args["pos"] == "pos" and warm.args["lattice"] == "lattice" and warm.args["temperatures"] == 300.0
    expected = np.concatenate([dynamics.maxwell_boltzmann(m, 300.0, int(sd)) for m, sd in zip(masses, seeds)])
    assert np.array_equal(warm.args["velocities"].numpy(), expected) and np.array_equal(warm.args["masses"], np.concatenate(masses))
    assert [c for c in batch.calls] == [("evaluate", k, None) for k in range(4)]
    assert warm.calls == [(("forces", k), ("stresses", k), k == 3) for k in range(4)]
