"""Import-path shim: `myutils.vis_events` of the reference, on top of ebfi_amd.eventvis (see matplotlib_plot_events)."""
