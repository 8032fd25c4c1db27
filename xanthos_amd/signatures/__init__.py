from .signatures import COLUMNS, EXCEEDANCE, VARS, Signatures, exceedance_name, output_stem, probabilities, signature_rows  # noqa: F401
