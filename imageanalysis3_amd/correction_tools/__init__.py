"""correction_tools — filter / alignment / translate operators (reference: correction_tools/)."""

_drift_channel = '488'
