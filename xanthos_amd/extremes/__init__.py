from .extremes import COLUMNS, KINDS, RETURN_PERIODS, VARS, Extremes, extremes_rows, output_stem  # noqa: F401
