"""Scoring the picks against known centres (mirror of the reference's cet_pick/evaluation)."""
from .algorithms import match_coordinates, match_coordinates_batch  # noqa: F401
from .metrics import precision_recall_curve  # noqa: F401
