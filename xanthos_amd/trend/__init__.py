from .trend import ANNUAL_DEFAULT, COLUMNS, SERIES, VARS, Trend, output_stem, trend_rows, z_of  # noqa: F401
