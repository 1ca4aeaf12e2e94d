"""FitEngine._route: which path serves each chi^2 request of a search round, and the books of the re-basing rule.

_route makes no library call, so these run on an engine made by __new__ with its state set by hand: no device, no
context.  Every expected mask, order and midpoint below is written out from the rule's own statement (the docstrings of
_route, _wants_rebase and _chi2_batch_search_raw), not taken from a run.
"""
import numpy as np
import pytest

from volumetricinterp_amd.fitengine import FitEngine

SWITCHES = ('WARM', 'SHAREDWALK', 'REBASE', 'REBASE2', 'REBASE_SCHEDULE', 'LPT')


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv('VINTERP_' + k, raising=False)


def _engine(T, ref=False, slots=()):
    e = FitEngine.__new__(FitEngine)
    e.N, e.P, e.T = 144, 500, T
    e.regularization_list = ['curvature']
    e.stats = dict(solves=0, launches=0)
    e._ref_rec = T if ref else None
    e._warm_reset()
    for r in slots:
        e._warm_slot[r] = len(e._warm_slot)
        e._basis_x[r] = -28.5
    return e


def _route(e, rec, x, forced=None):
    rec = np.asarray(rec, dtype=np.int32)
    x = np.asarray(x, dtype=np.float64)
    forced = np.zeros(len(rec), dtype=bool) if forced is None else np.asarray(forced, dtype=bool)
    cold, shared, warm, rebase, order, need = e._route(rec, x, forced)
    for m in (cold, shared, warm, rebase):
        assert m.dtype == bool and m.shape == rec.shape
    assert np.array_equal(cold.astype(int) + shared + warm + rebase, np.ones(len(rec), dtype=int))   # one path per request
    assert sorted(order.tolist()) == list(range(len(rec)))
    return cold.tolist(), shared.tolist(), warm.tolist(), rebase.tolist(), order.tolist(), need


def _books(e):
    return dict(e._last_x), dict(e._nreq), dict(e._rebased), dict(e._basis_x)


def test_walk_requests_without_a_reference_record_are_cold():
    e = _engine(4)
    cold, shared, warm, rebase, order, need = _route(e, [0, 1, 2, 3, 0, 1], [0., 0., 0., 0., -1., -1.])
    assert cold == [True] * 6 and not any(shared) and not any(warm) and not any(rebase)
    assert order == [0, 1, 2, 3, 4, 5]
    assert need == {} and _books(e) == ({}, {}, {}, {})


def test_walk_requests_with_a_reference_record_are_shared_and_sorted_by_decade(monkeypatch):
    e = _engine(8, ref=True)
    x = [-1., -3., -2., -3., -1., -2.]
    cold, shared, warm, rebase, order, need = _route(e, [0, 0, 0, 1, 1, 1], x)
    assert shared == [True] * 6 and not any(cold) and not any(warm) and not any(rebase)
    assert order == [1, 3, 2, 5, 0, 4]          # decade -3, -2, -1; requests of one decade in the order they came
    assert need == {} and _books(e) == ({}, {}, {}, {})
    # the shared walk needs its switch, eight records and the reference record
    monkeypatch.setenv('VINTERP_SHAREDWALK', '0')
    assert _route(e, [0, 0, 0, 1, 1, 1], x)[0] == [True] * 6
    monkeypatch.delenv('VINTERP_SHAREDWALK')
    e.T = 7
    assert _route(e, [0, 0, 0, 1, 1, 1], x)[0] == [True] * 6
    assert _route(_engine(8), [0, 0, 0, 1, 1, 1], x)[0] == [True] * 6


def test_forced_requests_go_cold_and_leave_the_books_alone():
    # `forced` is what _chi2_batch_search_raw makes of the search's `exact` requests and of _force_cold
    e = _engine(8, ref=True, slots=(2,))
    rec, x = [0, 1, 2, 2, 3], [-4., -4., -28.25, -28.26, -5.]
    cold, shared, warm, rebase, order, need = _route(e, rec, x, forced=[True, False, True, False, False])
    assert cold == [True, False, True, False, False]
    assert shared == [False, True, False, False, True]
    assert warm == [False, False, False, True, False] and not any(rebase)
    assert order == [0, 2, 4, 1, 3]             # cold, shared by decade (-5 before -4), warm
    assert need == {}
    assert _books(e) == ({2: -28.26}, {2: 1}, {}, {2: -28.5})      # the forced request of record 2 does not count


def test_first_root_finder_request_puts_the_basis_at_the_middle_of_the_unit_bracket():
    e = _engine(3)
    cold, shared, warm, rebase, order, need = _route(e, [2, 0, 1], [-28.3, -5.999, 0.25])
    assert warm == [True] * 3 and not any(cold) and not any(shared) and not any(rebase)
    assert order == [0, 1, 2]
    assert need == {0: -5.5, 1: 0.5, 2: -28.5} and list(need) == [0, 1, 2]        # sorted by record
    last, nreq, rebased, basis = _books(e)
    assert last == {2: -28.3, 0: -5.999, 1: 0.25} and nreq == {0: 1, 1: 1, 2: 1} and rebased == {}
    assert all(basis.get(r, need[r]) == need[r] for r in need)     # nobody has put the basis anywhere else


def test_several_requests_of_a_record_in_one_round():
    # a multisection round: the midpoint comes from the first request, the re-basing rule does not see the round
    e = _engine(2)
    cold, shared, warm, rebase, order, need = _route(e, [0, 0, 0, 1, 1], [-7.75, -7.5, -7.25, -3.2, -3.7])
    assert warm == [True] * 5 and not any(rebase)
    assert need == {0: -7.5, 1: -3.5}
    assert _books(e)[:3] == ({}, {}, {})
    # ... nor when the record has its rotated system and a previous request right next to these
    e = _engine(2, slots=(0,))
    e._last_x[0], e._nreq[0] = -7.5001, 3
    cold, shared, warm, rebase, order, need = _route(e, [0, 0], [-7.5, -7.5002])
    assert warm == [True, True] and not any(rebase) and need == {}
    assert _books(e) == ({0: -7.5001}, {0: 3}, {}, {0: -28.5})


def test_a_request_next_to_the_previous_one_moves_the_basis_exactly_once():
    e = _engine(2, slots=(0, 1))
    w = FitEngine.REBASE_WITHIN
    assert _route(e, [0, 1], [-28.2, -28.8])[2:4] == ([True, True], [False, False])      # no previous request yet
    # record 0 comes within REBASE_WITHIN of its previous request, record 1 does not
    cold, shared, warm, rebase, order, need = _route(e, [0, 1], [-28.2 + 0.9 * w, -28.8 + 1.1 * w])
    assert warm == [False, True] and rebase == [True, False] and order == [1, 0] and need == {}
    last, nreq, rebased, basis = _books(e)
    assert rebased == {0: 1} and basis == {0: -28.2 + 0.9 * w, 1: -28.5}
    assert last == {0: -28.2 + 0.9 * w, 1: -28.8 + 1.1 * w} and nreq == {0: 2, 1: 2}
    # closer still: record 0 has had its move, record 1 has its own now
    cold, shared, warm, rebase, order, need = _route(e, [0, 1], [-28.2 + 0.91 * w, -28.8 + 1.2 * w])
    assert warm == [True, False] and rebase == [False, True] and order == [0, 1]
    assert e._rebased == {0: 1, 1: 1} and e._basis_x == {0: -28.2 + 0.9 * w, 1: -28.8 + 1.2 * w}
    assert _route(e, [0, 1], [-28.2 + 0.911 * w, -28.8 + 1.21 * w])[3] == [False, False]
    assert e._rebased == {0: 1, 1: 1} and e._nreq == {0: 4, 1: 4}


def test_the_second_move_after_many_requests(monkeypatch):
    n, w2 = FitEngine.REBASE_AGAIN_AFTER, FitEngine.REBASE_AGAIN_WITHIN

    def engine(nreq, rebased=1):
        e = _engine(1, slots=(0,))
        e._last_x[0], e._nreq[0], e._rebased[0] = -28.4, nreq, rebased
        return e
    assert _route(engine(n - 1), [0], [-28.4 + 0.5 * w2])[3] == [False]           # too few requests so far
    assert _route(engine(n), [0], [-28.4 + 2 * w2])[3] == [False]                 # not close enough
    assert _route(engine(n, rebased=0), [0], [-28.4 + 2 * w2])[3] == [True]       # (that is the first move's distance)
    e = engine(n)
    assert _route(e, [0], [-28.4 + 0.5 * w2])[3] == [True]
    assert _books(e) == ({0: -28.4 + 0.5 * w2}, {0: n + 1}, {0: 2}, {0: -28.4 + 0.5 * w2})
    assert _route(e, [0], [-28.4 + 0.6 * w2])[2:4] == ([True], [False])           # and never a third
    assert e._rebased == {0: 2} and e._nreq == {0: n + 2}
    monkeypatch.setenv('VINTERP_REBASE2', '0')
    assert _route(engine(n), [0], [-28.4 + 0.5 * w2])[3] == [False]


def test_rebase_switched_off(monkeypatch):
    monkeypatch.setenv('VINTERP_REBASE', '0')
    e = _engine(1, slots=(0,))
    _route(e, [0], [-28.2])
    cold, shared, warm, rebase, order, need = _route(e, [0], [-28.2 + 1e-9])
    assert warm == [True] and rebase == [False]
    assert _books(e) == ({0: -28.2 + 1e-9}, {0: 2}, {}, {0: -28.5})


def test_a_mixed_round_and_the_order_of_a_big_warm_launch(monkeypatch):
    e = _engine(8, ref=True, slots=(0, 1))
    e._last_x[1], e._nreq[1] = -28.3, 1
    #      walk        exact end  warm      rebase    walk   first request of record 5
    rec = [3, 4, 3, 0, 1, 2, 5]
    x = [-2., -1., -2., -28.7, -28.301, -3., -6.5]
    forced = [False, False, True, False, False, False, False]
    cold, shared, warm, rebase, order, need = _route(e, rec, x, forced)
    assert (cold, shared) == ([False, False, True, False, False, False, False], [True, True, False, False, False, True, False])
    assert (warm, rebase) == ([False, False, False, True, False, False, True], [False, False, False, False, True, False, False])
    assert order == [2, 5, 0, 1, 3, 6, 4] and need == {5: -6.5}
    # more than 256 warm requests: furthest from the record's basis first (equal distances in the order they came)
    n = 300
    e = _engine(n, slots=range(1, n))                   # bases at -28.5; record 0 gets its at -28.5 in this round
    xs = -28.5 + (np.arange(n) % 7) * 0.01 * np.where(np.arange(n) % 2, 1., -1.) + 1e-3
    dist = np.abs(xs + 28.5)
    order = _route(e, np.arange(n), xs)[4]
    assert order == np.argsort(-dist, kind='stable').tolist() and len(set(order[:10])) == 10
    monkeypatch.setenv('VINTERP_LPT', '0')
    assert _route(_engine(n, slots=range(1, n)), np.arange(n), xs)[4] == list(range(n))
    monkeypatch.delenv('VINTERP_LPT')
    assert _route(_engine(256, slots=range(256)), np.arange(256), xs[:256])[4] == list(range(256))      # 256: as they came
