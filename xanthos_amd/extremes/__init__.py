from .extremes import CI_COLUMNS, COLUMNS, KINDS, RETURN_PERIODS, VARS, Extremes, bootstrap_rows, extremes_rows, output_stem  # noqa: F401
