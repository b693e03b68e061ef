"""The launch order of every u16 route is the recorded one (tests/golden/launch_order_u16.json, written by tests/launchorder.py from the
library as it stood before the chain's host code was split into route functions).  The other GPU tests check which kernels a route
ran; this one pins their ORDER, `host:` segments and the stripes' all-reduces included, route by route.  Launches without a timer of
their own (the verdict, the remap, the recount behind the guard) do not show here: their place is read off the route functions."""
import json
import os

import pytest

import launchorder

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_order_u16.json")) as f:
    GOLDEN = json.load(f)


def test_every_route_has_a_recorded_order():
    assert sorted(GOLDEN) == sorted(launchorder.ROUTES)


@pytest.mark.parametrize("route", sorted(launchorder.ROUTES))
def test_launch_order_is_the_recorded_one(route):
    got = launchorder.run_route(route)
    assert got == GOLDEN[route], route
