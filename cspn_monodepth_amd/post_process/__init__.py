"""Mirror of the reference package network/libs/post_process (CSPN, CSPN_new, CSPN_ours)."""
from . import CSPN, CSPN_new, CSPN_ours
from .CSPN_new import AffinityPropagate

__all__ = ["CSPN", "CSPN_new", "CSPN_ours", "AffinityPropagate"]
