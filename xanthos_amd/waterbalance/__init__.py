from .waterbalance import COLUMNS, LEVELS, OMEGA0, WaterBalance, balance_rows, basin_rows, csv_columns, output_stem  # noqa: F401
