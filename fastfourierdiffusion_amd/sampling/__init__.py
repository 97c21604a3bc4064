from .forecast import ensemble_scores  # noqa: F401
